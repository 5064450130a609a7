// What every host-side context (the engine, the towers) shares: status plumbing and the C-ABI glue, the weight registry, one weight as a
// record, workspace carving, the plain GEMM parameter block and its launch, the SAMAUDIO_OPT_X3_CLASSES launch vocabulary.  Host code
// only - no kernel source includes this.
#pragma once
#include <cstdint>
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

inline Status fail(int code, const std::string& m) { return Status{code, m}; }
inline long round_up(long v, long m) { return (v + m - 1) / m * m; }

// The C entry points: a Status into its return code (the message behind samaudio_last_error()), an argument error, and the usual
// body - a null handle is `what`, anything else the call's Status
inline int ret(const Status& s) {
  if (!s.ok()) set_last_error(s.msg);
  return s.code;
}
inline int bad(const char* msg) {
  set_last_error(msg);
  return SAMAUDIO_ERR_ARG;
}
#define SA_ENTRY(handle, what, call) ((handle) ? sa::ret(call) : sa::bad(what))

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

// finalize: the fp32 tensor / the GEMM-operand tensor (of dtype `at`) `name` of the registry `reg` into `field`
#define NEEDF(reg, field, name, ...) SA_TRY((reg).need(name, SAMAUDIO_DT_F32, {__VA_ARGS__}, (const void**)&(field)))
#define NEEDW(reg, at, field, name, ...) SA_TRY((reg).need(name, at, {__VA_ARGS__}, (const void**)&(field)))

class Bump {  // workspace carving (also used dry to size the workspace)
 public:
  explicit Bump(char* base = nullptr, size_t cap = 0) : base_(base), cap_(cap) {}
  void* take(size_t bytes) {
    size_t off = (used_ + 255) & ~size_t(255);
    used_ = off + bytes;
    return base_ ? base_ + off : nullptr;
  }
  size_t used() const { return (used_ + 255) & ~size_t(255); }
  bool fits() const { return used() <= cap_; }
  void reset_to(size_t mark) { used_ = mark; }
  size_t mark() const { return used_; }

 private:
  char* base_;
  size_t cap_;
  size_t used_ = 0;
};

// the plain launch C[M, N] = A[M, K] W[N, K]^T: one batch, one K block, alpha 1
inline GemmParams lin(const void* A, long lda, const void* W, long M, int N, int K) {
  GemmParams p;
  std::memset(&p, 0, sizeof(p));
  p.A = A; p.W = W; p.lda = lda; p.kc = K; p.tap_stride = 0;
  p.M = (int)M; p.N = N; p.K = K; p.nbatch = 1; p.alpha = 1.f; p.rows_per_gate = 1;
  return p;
}

// gemm_check + launch_gemm; `who`: the context's prefix of the refusal ("" for the PE-AV towers)
inline Status run_gemm(const GemmParams& p, bool bf16, const char* who, hipStream_t st) {
  if (const char* why = gemm_check(p, bf16)) return fail(SAMAUDIO_ERR_ARG, std::string(who) + why);
  SA_HIP(launch_gemm(p, bf16, st));
  return Status{};
}

// SAMAUDIO_OPT_X3_CLASSES, shared by the DiT engine and the towers.
// A launch stated on an fp32 tensor, restated on that tensor's split copy (every element of the K axis became three): the one place
// offsets, strides and extents along K are scaled.  It does not say how K' is laid out - the two functions below do, and the caller
// picks one (a helper that infers it was the bug)
inline void x3_scale_k(GemmParams& p) { p.a_off *= 3; p.a_bstride *= 3; p.lda *= 3; p.tap_stride *= 3; p.kc *= 3; p.K *= 3; }
// K' split per input block (the k3 convolutions: a tap is [lo | hi | hi] of a row against that tap's [W_hi | W_lo | W_hi]; the codec's
// wide convolutions: per Cin-block): the geometry of `p` on the split buffer `a3`.  A plain walk over K' - never x3_share
inline void x3_block_operands(GemmParams& p, const void* a3, const void* w3, bool ktm3) {
  p.A = a3; p.W = w3;
  x3_scale_k(p);
  if (ktm3) p.flags |= GEMM_FLAG_W_KTM;
}
// K' split over the whole K: the 16-bit launch over K' = 3K that an x3 class makes of its fp32 GemmParams (kc == K, no taps).
// A = the split operand [lo | hi | hi] (dense rows of 3K; a batched launch keeps its offsets, into the split copy of the same tensor),
// W = the split weight [W_hi | W_lo | W_hi]
inline void x3_operands(GemmParams& p, const void* a3, const LinW& w) {
  p.lda = p.K;
  x3_block_operands(p, a3, w.w3, w.ktm3);
  if (p.out_act) {   // an fp32 context's "activation" outputs are fp32 tensors: the 16-bit kernel writes them as its fp32 output
    p.out_f32 = (float*)p.out_act; p.f32_ld = p.act_ld; p.f32_bstride = p.act_bstride; p.f32_off = p.act_off;
    p.f32_act = p.act != ACT_NONE;
    p.out_act = nullptr; p.act_ld = p.act_bstride = p.act_off = 0;
  }
  if ((p.flags & GEMM_FLAG_OUT_SPLIT3) && p.out_f32) {   // the result leaves as the next GEMM's split operand (16-bit, 3 x n_out per row)
    p.out_act = p.out_f32; p.act_ld = 3L * (p.swiglu ? p.N / 2 : p.N); p.act_bstride = p.act_off = 0;
    p.out_f32 = nullptr; p.f32_ld = p.f32_bstride = p.f32_off = 0; p.f32_act = 0;
  }
}
// An x3 launch on K-concatenated split operands: let the 8-phase kernels share the operand tiles the three products have in common
// (common.h GEMM_FLAG_X3_SHARE) wherever the launch qualifies; DBG_X3_PLAIN_WALK = 1: the plain walk over K' (A/B, tests), >= 2: a class
// mask << 1 that keeps the sharing order for those classes only (diagnosis).  Launches with K' split per input block (the
// convolutions) never come here.
inline GemmParams x3_share(const GemmParams& p, int cls) {
  const int plain_walk = debug_flag(DBG_X3_PLAIN_WALK);
  if (plain_walk == 1 || (plain_walk >= 2 && !(cls & (plain_walk >> 1)))) return p;
  GemmParams q = p;
  q.flags |= GEMM_FLAG_X3_SHARE;
  return q.kc == q.K && q.K % 192 == 0 && !gemm_check(q, true) ? q : p;
}

// The launch of `p` (an x3 class's fp32 launch on the split operand a3) that writes its result as the NEXT GEMM's split operand into
// `out3`: the caller finishes it the way it launches (launch_params / x3_share) and asks gemm_check whether the 8-phase family takes it
inline GemmParams x3_split3_out(GemmParams p, const void* a3, const LinW& w, void* out3) {
  p.out_act = out3;
  p.flags |= GEMM_FLAG_OUT_SPLIT3;
  x3_operands(p, a3, w);
  return p;
}
// `rows` split rows of 3 k 16-bit elements fit the scratch `buf` of `cap` bytes; x3_fits: ... or `who` + `what`, the context's message
inline bool x3_room(const void* buf, size_t cap, long rows, long k) { return buf && (size_t)rows * 3 * k * 2 <= cap; }
inline Status x3_fits(const void* buf, size_t cap, long rows, long k, const std::string& who, const char* what) {
  return x3_room(buf, cap, rows, k) ? Status{} : Status{SAMAUDIO_ERR_WORKSPACE, who + "SAMAUDIO_OPT_X3_CLASSES: " + what};
}

// "a plain whole-K launch with one output": what an x3 class can restate on operands split over the whole K (x3_operands), and the
// only form that may take the sharing walk.  Asked here and nowhere else
inline bool x3_whole_k(const GemmParams& p) { return p.kc == p.K && !p.tap_stride && !(p.out_act && p.out_f32); }

// Where the split A operand of an x3 launch comes from: `split` = already split by its producer, else "split the fp32 rows here into
// this scratch of this capacity".  per_tap: a k3 convolution on a split halo buffer - K' split per tap, the plain walk (never shares)
struct X3Operand { const void* split; void* scratch; size_t bytes; bool per_tap = false; };

// One launch of a tower context on the weight `w`: `p` = the context's plain launch, run as it is on w.w (operands `bf16`) - or, class
// `cls` switched to compensated operands (`on`), as ONE 16-bit launch over K' = 3K on w.w3 and the split operand `a` names.  `who`
// prefixes the context's own messages, `gemm_who` what gemm_check refuses (run_gemm); both are read on a failing path only
inline Status x3_linear(GemmParams p, const LinW& w, int cls, bool on, bool bf16, const X3Operand& a, const char* who,
                        const char* gemm_who, hipStream_t st) {
  p.W = w.w;
  if (!on) return run_gemm(p, bf16, gemm_who, st);
  if (!w.w3) return fail(SAMAUDIO_ERR_STATE, std::string(who) + "SAMAUDIO_OPT_X3_CLASSES: split weight missing (set the option before finalize)");
  if (a.per_tap) {   // the caller said so: K' split per tap, no operand sharing
    x3_block_operands(p, a.split, w.w3, w.ktm3);
    return run_gemm(p, true, gemm_who, st);
  }
  if (!x3_whole_k(p)) return fail(SAMAUDIO_ERR_ARG, std::string(who) + "SAMAUDIO_OPT_X3_CLASSES: plain launches with one output only");
  const void* split = a.split;
  if (!split) {   // split the fp32 rows here (an operand no kernel wrote in split form)
    if (p.nbatch != 1 || p.a_off) return fail(SAMAUDIO_ERR_ARG, std::string(who) + "SAMAUDIO_OPT_X3_CLASSES: a batched operand must arrive split");
    if (!x3_room(a.scratch, a.bytes, p.M, p.K))   // (the message is built on this path only)
      return x3_fits(a.scratch, a.bytes, p.M, p.K, who, "the split operand does not fit the scratch the workspace plan holds");
    SA_HIP(launch_split3((const float*)p.A, p.lda, a.scratch, p.M, p.K, st));
    split = a.scratch;
  }
  x3_operands(p, split, w);
  return run_gemm(x3_share(p, cls), true, gemm_who, st);
}

// The tag / flags a context launches `p_in` with.  From the caller: alt-format output, K-tile-major W, split-form output; from the
// context: the kernel symbols (`tag` 1: the codec's), the tail split (gemm.hip gemm_tail_split), operands in the alt format.
// `share_cls` >= 0: an x3 launch on operands split over the whole K - it shares operand tiles wherever it qualifies (x3_share)
inline GemmParams gemm_launch_params(const GemmParams& p_in, int tag, bool tail_split, bool opnd_alt, int share_cls) {
  GemmParams p = p_in;
  p.tag = tag;
  p.flags = (p_in.flags & (GEMM_FLAG_OUT_ALT | GEMM_FLAG_W_KTM | GEMM_FLAG_OUT_SPLIT3)) | (tail_split ? 0 : GEMM_FLAG_NO_TAIL_SPLIT) |
            (opnd_alt ? GEMM_FLAG_OPND_ALT : 0);
  return share_cls >= 0 ? x3_share(p, share_cls) : p;
}

// ---- SAMAUDIO_OPT_X3_CLASSES bit CODEC: the geometry of one DAC-VAE convolution of an fp32 context ------------------------------
// The engine (codec_gemm / gemm_codec_x3) and the test hook (api.hip samaudio_op_codec_conv) both launch by these functions: there
// is no second statement of the strides anywhere.
//
// The narrow form: the fp32 kernel splits its operands in registers (GEMM_FLAG_X3_FLY); `fly` = the weight's "<name>.fly" twin
// (already split, GEMM_FLAG_W_FLY16) or null.  `p` = the launch as launch_params left it
inline void codec_fly_operands(GemmParams& p, const void* fly) {
  p.flags |= GEMM_FLAG_X3_FLY;
  if (fly && !p.w_bstride) { p.W = fly; p.flags |= GEMM_FLAG_W_FLY16; }
}
// The wide form (N >= 256, a "<name>.x3" twin with Cin-blocks of `c` channels): can `p` run on the buffer split row by row into a
// scratch of `scratch_bytes`?  Every K-axis quantity must be whole input rows; the activation pass (codec_x3_act) walks ONE contiguous
// region per item with the raw stream's geometry, so both outputs must be dense rows of N (a windowed launch: identical geometry)
inline bool codec_x3_eligible(const GemmParams& p, int c, size_t scratch_bytes) {
  if (p.N < 256 || c <= 0) return false;
  const bool both = p.out_f32 && p.out_act;
  const bool flat = (!p.out_f32 || p.f32_ld == p.N) && (!p.out_act || p.act_ld == p.N) && (!p.c_ld_rel || p.c_ld_rel == p.N);
  return p.a_bstride > 0 && !p.w_bstride && !p.swiglu && !p.gate && !(p.kc % c) && !(p.lda % c) && !(p.a_off % c) &&
         !(p.a_bstride % c) && !(p.tap_stride % c) && !(p.K % c) && !((3L * p.K) % 64) && flat && (!both || !p.f32_act) &&
         (size_t)p.nbatch * (p.a_bstride / c) * 3 * c * 2 <= scratch_bytes;
}
// every row of the halo buffers the launch reads (halo rows are zeros): what launch_split3 splits into the scratch, `c` wide
inline long codec_x3_split_rows(const GemmParams& p, int c) { return (long)p.nbatch * (p.a_bstride / c); }
// whole-K (a k1 convolution on one block: operands split over the whole K, may share operand tiles) or per input block (a plain walk)
inline bool codec_x3_whole_k(const GemmParams& p, int c) { return p.K == c && p.kc == c; }
// The 16-bit launch over K' = 3K on the split buffer `a3` and the twin `w3`.  It writes the RAW fp32 result - into the raw stream, or
// (a launch with an activated output only) into that buffer; the activation follows as an elementwise pass (codec_x3_act)
inline GemmParams codec_x3_launch(const GemmParams& p_in, const void* a3, const void* w3) {
  GemmParams p = p_in;
  x3_block_operands(p, a3, w3, false);   // ("one block": the whole K' is one [lo | hi | hi] x [W_hi | W_lo | W_hi])
  if (!p_in.out_f32) { p.out_f32 = (float*)p_in.out_act; p.f32_ld = p_in.act_ld; p.f32_bstride = p_in.act_bstride; p.f32_off = p_in.act_off; }
  p.out_act = nullptr; p.act_ld = p.act_bstride = p.act_off = 0; p.act = ACT_NONE; p.f32_act = 0;
  return p;
}
// The activation pass behind codec_x3_launch: act(raw) over the region the launch wrote, per item - [c_lo, c_hi) of the windowed
// (transposed) convolutions, else M rows of N.  run = false: the launch needs none; aligned = false: the window does not start on a
// whole channel row (refused - act_flat_kernel takes its channel from the index inside the region)
struct CodecActPass {
  bool run, aligned;
  const float* in; long in_bstride;
  float* out; long out_bstride;
  int items; long count; int chan, act;
  const float* alpha;
};
inline CodecActPass codec_x3_act(const GemmParams& p) {
  CodecActPass a{};
  a.run = p.out_act && !(p.act == ACT_NONE && !p.out_f32);
  if (!a.run) return a;
  const float* const raw = p.out_f32 ? p.out_f32 : (const float*)p.out_act;
  const long raw_off = p.out_f32 ? p.f32_off : p.act_off;
  const long start = p.c_ld_rel ? p.c_lo : 0;
  a.count = p.c_ld_rel ? p.c_hi - p.c_lo : (long)p.M * p.N;
  a.chan = p.chan_mod ? p.chan_mod : p.N;
  a.aligned = start % a.chan == 0;
  a.in = raw + raw_off + start; a.in_bstride = p.out_f32 ? p.f32_bstride : p.act_bstride;
  a.out = (float*)p.out_act + p.act_off + start; a.out_bstride = p.act_bstride;
  a.items = p.nbatch; a.act = p.act; a.alpha = p.act_alpha;
  return a;
}

// Can the up-projection `up` (an x3 class's fp32 launch on the split operand a3, M rows) write the down-projection's split operand
// [M, 3F] into `out3` itself?  The scratch holds it and gemm_check takes the launch that `finish` makes of it - the caller's own way
// of launching (the engine: launch_params(.., GemmKind::X3); the towers: x3_share).  Otherwise the down-projection splits the fp32
// hidden with launch_split3
template <class Finish>
inline bool x3_w2_pre(const GemmParams& up, const void* a3, const LinW& w, void* out3, size_t cap, long M, long F, Finish&& finish) {
  return x3_room(out3, cap, M, F) && !gemm_check(finish(x3_split3_out(up, a3, w, out3)), true);
}

}  // namespace sa
