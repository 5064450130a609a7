// What every host-side context (the engine, the towers) shares: status plumbing, the weight registry, one weight as a record, the
// plain GEMM parameter block.  Host code only - no kernel source includes this.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/samaudio.h"
#include "kernels.h"

namespace sa {

struct TensorRef {
  const void* p = nullptr;
  int dtype = 0;
  std::vector<int64_t> shape;
};

struct Status {
  int code = 0;
  std::string msg;
  bool ok() const { return code == 0; }
};

void set_last_error(const std::string& msg);  // api.hip: the thread-local string behind samaudio_last_error()

#define SA_TRY(expr)                     \
  do {                                   \
    sa::Status _s = (expr);              \
    if (!_s.ok()) return _s;             \
  } while (0)
#define SA_HIP(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return sa::Status{SAMAUDIO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)}; \
  } while (0)

struct LinW {             // one linear / convolution weight as a context resolved it
  const void* w = nullptr;   bool ktm = false;    // native operand; K-tile-major [K/64][N][64]
  const void* w3 = nullptr;  bool ktm3 = false;   // "<name>.x3" twin [W_hi | W_lo | W_hi]; null = not registered
};

class Registry {  // name -> borrowed weight tensor
 public:
  Status set(const char* name, const void* p, int dtype, int ndim, const int64_t* shape);
  const TensorRef* find(const std::string& name) const;
  bool has(const std::string& name) const { return find(name) != nullptr; }
  const std::map<std::string, TensorRef>& all() const { return tensors_; }
  Status need(const std::string& name, int dtype, std::vector<int64_t> shape, const void** out) const;
  // SAMAUDIO_OPT_X3_CLASSES: the 16-bit split twin "<name>" of a weight, [N, K3] row-major or K-tile-major [K3 / 64, N, 64], into
  // w.w3 / w.ktm3.  twin: null where it is not registered in either shape (the engine checks when a class is switched on);
  // need_twin: SAMAUDIO_ERR_WEIGHT names it (the towers resolve at finalize)
  void twin(const std::string& name, int64_t N, int64_t K3, LinW& w) const;
  Status need_twin(const std::string& name, int64_t N, int64_t K3, LinW& w) const;

 private:
  std::map<std::string, TensorRef> tensors_;
};

// the plain launch C[M, N] = A[M, K] W[N, K]^T: one batch, one K block, alpha 1
inline GemmParams lin(const void* A, long lda, const void* W, long M, int N, int K) {
  GemmParams p;
  std::memset(&p, 0, sizeof(p));
  p.A = A; p.W = W; p.lda = lda; p.kc = K; p.tap_stride = 0;
  p.M = (int)M; p.N = N; p.K = K; p.nbatch = 1; p.alpha = 1.f; p.rows_per_gate = 1;
  return p;
}

}  // namespace sa
