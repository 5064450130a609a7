// Engine: sequences the HIP kernels of SAMAudio.separate() (reference sam_audio/model/model.py:247-338).
// Host code only - every arithmetic step is a kernel from gemm.hip / kernels.hip / attention.hip.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sa {

// SAMAUDIO_TRACE=1: after each stage of an evaluation, synchronise, copy the stage's buffer to the host and print how
// many values are non-finite plus the largest magnitude (debugging aid; never on in timed runs).
static bool trace_on() {
  static const bool on = std::getenv("SAMAUDIO_TRACE") != nullptr;
  return on;
}
// SAMAUDIO_TRACE_HASH=1: the same stages, WITHOUT synchronising: a checksum kernel per stage writes one 64-bit word per batch
// item into a debug buffer on the launch stream; ode_solve / forward print them afterwards ("[samaudio hash] <context>
// <sequence> <stage> item <b> <hex>").  Two runs whose rows must agree (one stream vs two streams, whole batch vs shards)
// are compared stage by stage offline (tools/diag_hash.py): the first stage whose checksums differ names the kernel.
// Debugging aid; the only place the library allocates device memory (hipMalloc of 8 MiB, on first use).
struct HashTrace {
  struct Rec { std::string name; int items; size_t slot; };
  unsigned long long* dev = nullptr;
  size_t used = 0, seq = 0;
  std::vector<Rec> recs;
  static constexpr size_t CAP = 1 << 20;
  bool full_warned = false;
};
// eval_field sets the running context's recorder for the duration of ONE evaluation: cleared on every way out, so that a later
// trace() on this thread (the codec, another context) cannot append to this context's recorder
struct HashScope {
  explicit HashScope(HashTrace* h, int items);
  ~HashScope();
};
static bool hash_on() {
  static const bool on = std::getenv("SAMAUDIO_TRACE_HASH") != nullptr;
  return on;
}
static thread_local HashTrace* g_hash = nullptr;   // the running context's recorder (set by eval_field)
static thread_local int g_hash_items = 1;
HashScope::HashScope(HashTrace* h, int items) { g_hash = h; g_hash_items = items; }
HashScope::~HashScope() { g_hash = nullptr; g_hash_items = 1; }
static void hash_stage(const char* name, const void* dev, size_t bytes, hipStream_t st) {
  HashTrace* h = g_hash;
  if (!h || !dev || bytes < 4) return;
  if (!h->dev && !(h->dev = (unsigned long long*)debug_device_alloc(HashTrace::CAP * 8))) return;
  int items = g_hash_items;
  if (items <= 0 || (bytes / 4) % (size_t)items) items = 1;
  if (h->used + items > HashTrace::CAP) {
    if (!h->full_warned) std::fprintf(stderr, "[samaudio hash] recorder full (%zu words): later stages are NOT recorded\n", HashTrace::CAP);
    h->full_warned = true;
    return;
  }
  (void)launch_hash_items((const unsigned*)dev, bytes / 4 / items, items, h->dev + h->used, st);
  h->recs.push_back({name, items, h->used});
  h->used += items;
}
static void hash_flush(HashTrace* h, const void* ctx, hipStream_t st) {
  if (!h || !h->dev || h->recs.empty()) return;
  (void)hipStreamSynchronize(st);
  std::vector<unsigned long long> host(h->used);
  if (hipMemcpy(host.data(), h->dev, h->used * 8, hipMemcpyDeviceToHost) == hipSuccess)
    for (const auto& r : h->recs) {
      for (int b = 0; b < r.items; ++b)
        std::fprintf(stderr, "[samaudio hash] %p %zu %s item %d of %d %016llx\n", ctx, h->seq, r.name.c_str(), b, r.items,
                     host[r.slot + b]);
      ++h->seq;
    }
  h->recs.clear();
  h->used = 0;
}

static void trace(const char* name, const void* dev, size_t count, bool is_bf16, hipStream_t st) {
  if (hash_on()) hash_stage(name, dev, count * (is_bf16 ? 2 : 4), st);
  if (!trace_on() || !dev || !count) return;
  (void)hipStreamSynchronize(st);
  std::vector<unsigned char> host(count * (is_bf16 ? 2 : 4));
  if (hipMemcpy(host.data(), dev, host.size(), hipMemcpyDeviceToHost) != hipSuccess) return;
  size_t bad = 0;
  double mx = 0.0;
  for (size_t i = 0; i < count; ++i) {
    float v;
    if (is_bf16) {
#ifdef SA_OPERAND_FP16
      const unsigned short hw = ((const unsigned short*)host.data())[i];
      const int e = (hw >> 10) & 31, m = hw & 1023;
      const float mag = e == 31 ? (m ? NAN : INFINITY) : (e ? std::ldexp(1.f + m / 1024.f, e - 15) : std::ldexp(m / 1024.f, -14));
      v = (hw & 0x8000) ? -mag : mag;
#else
      const unsigned u = (unsigned)((const unsigned short*)host.data())[i] << 16;
      std::memcpy(&v, &u, 4);
#endif
    } else {
      v = ((const float*)host.data())[i];
    }
    if (!std::isfinite(v)) ++bad;
    else if (std::fabs(v) > mx) mx = std::fabs(v);
  }
  std::fprintf(stderr, "[samaudio trace] %-22s n=%zu non-finite=%zu max|x|=%.4g\n", name, count, bad, mx);
}

Engine::Engine(const samaudio_config& c) : cfg_(c) {
  bf16_ = c.precision == SAMAUDIO_BF16;
  esz_ = bf16_ ? 2 : 4;
  at_dtype_ = bf16_ ? SAMAUDIO_DT_BF16 : SAMAUDIO_DT_F32;
  std::memset(&g32_, 0, sizeof(g32_));
  std::memset(&enc_, 0, sizeof(enc_));
  std::memset(&dec_, 0, sizeof(dec_));
  std::memset(&d_, 0, sizeof(d_));
}

// ---------------------------------------------------------------------------------------------------
// the weight registry (host.h): every context's name -> borrowed tensor map
// ---------------------------------------------------------------------------------------------------
Status Registry::set(const char* name, const void* p, int dtype, int ndim, const int64_t* shape) {
  if (!name || !p || ndim < 0 || ndim > 4) return fail(SAMAUDIO_ERR_ARG, "set_tensor: bad argument");
  if ((reinterpret_cast<uintptr_t>(p) & 15) != 0)
    return fail(SAMAUDIO_ERR_ARG, std::string("set_tensor: ") + name + " is not 16-byte aligned");
  TensorRef t;
  t.p = p;
  t.dtype = dtype;
  t.shape.assign(shape, shape + ndim);
  tensors_[name] = t;
  return Status{};
}

const TensorRef* Registry::find(const std::string& name) const {
  auto it = tensors_.find(name);
  return it == tensors_.end() ? nullptr : &it->second;
}

Status Registry::need(const std::string& name, int dtype, std::vector<int64_t> shape, const void** out) const {
  const TensorRef* t = find(name);
  if (!t) return fail(SAMAUDIO_ERR_WEIGHT, "missing weight tensor '" + name + "'");
  if (t->dtype != dtype) return fail(SAMAUDIO_ERR_WEIGHT, "weight '" + name + "' has the wrong dtype");
  if (t->shape != shape) {
    std::string s = "weight '" + name + "' has shape [";
    for (auto v : t->shape) s += std::to_string(v) + ",";
    s += "] expected [";
    for (auto v : shape) s += std::to_string(v) + ",";
    return fail(SAMAUDIO_ERR_WEIGHT, s + "]");
  }
  *out = t->p;
  return Status{};
}

void Registry::twin(const std::string& name, int64_t N, int64_t K3, LinW& w) const {
  const TensorRef* t = find(name);
  w.w3 = nullptr;
  w.ktm3 = t && t->dtype == SAMAUDIO_DT_BF16 && K3 % 64 == 0 && t->shape == std::vector<int64_t>{K3 / 64, N, 64};
  if (w.ktm3 || (t && t->dtype == SAMAUDIO_DT_BF16 && t->shape == std::vector<int64_t>{N, K3})) w.w3 = t->p;
}

Status Registry::need_twin(const std::string& name, int64_t N, int64_t K3, LinW& w) const {
  twin(name, N, K3, w);
  if (w.w3) return Status{};
  return fail(SAMAUDIO_ERR_WEIGHT, "SAMAUDIO_OPT_X3_CLASSES: the split weight '" + name + "' (16-bit, [" + std::to_string(N) + ", " +
                                       std::to_string(K3) + "] or [" + std::to_string(K3 / 64) + ", " + std::to_string(N) +
                                       ", 64]) of a class that is switched on is not registered");
}

Status Engine::set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape) {
  const bool known = name && reg_.has(name);
  SA_TRY(reg_.set(name, p, dtype, ndim, shape));
  // Re-registering a name invalidates the resolved pointers: finalize() must run again.  Adding new names
  // (e.g. the codec set after the DiT set) leaves an already finalized set valid.
  if (known) dit_ready_ = codec_ready_ = enc_ready_ = false;
  return Status{};
}

const void* Engine::opt(const std::string& name, std::vector<int64_t> shape) const {
  const TensorRef* t = reg_.find(name);
  return t && t->dtype == SAMAUDIO_DT_F32 && t->shape == shape ? t->p : nullptr;
}

Status Engine::need_w5(const std::string& name, int N, int K, LinW& w) const {
  const TensorRef* t = reg_.find(name);
  w.ktm = t && bf16_ && t->dtype == at_dtype_ && t->shape == std::vector<int64_t>{K / 64, N, 64} && K % 64 == 0;
  if (w.ktm) {
    w.w = t->p;
    return Status{};
  }
  return reg_.need(name, at_dtype_, {N, K}, &w.w);
}

static int kpad(int k, bool bf16) { return (int)round_up(k, bf16 ? 64 : 32); }

Status Engine::finalize(int what) {
  const int D = cfg_.dim, F = cfg_.ffn_hidden, L = cfg_.n_layers, C2 = cfg_.latent_channels;
  const int AT = at_dtype_;
  if (what == 0) {
    // head_dim = dim / n_heads: 128 (every kernel tuned for it) or 64 (general forms of qkv_prep / the norms / cross-attention,
    // the self-attention kernel's 64-wide instantiation, no folded cross-attention projection)
    if (D % 256 || cfg_.n_heads <= 0 || D % cfg_.n_heads || (D / cfg_.n_heads != 128 && D / cfg_.n_heads != 64))
      return fail(SAMAUDIO_ERR_ARG, "dim must be a multiple of 256 and dim / n_heads (the head width) 128 or 64");
    const int hd = D / cfg_.n_heads;
    if (F % 64 || C2 % 64 || cfg_.text_dim % 64 || cfg_.video_dim % 64 || cfg_.freq_dim % 64 || cfg_.anchor_dim % 64)
      return fail(SAMAUDIO_ERR_ARG, "channel widths must be multiples of 64");
    layers_.assign(L, LayerW{});
    for (int i = 0; i < L; ++i) {
      const std::string P = "L" + std::to_string(i) + ".";
      LayerW& w = layers_[i];
      NEEDF(reg_, w.attn_norm, P + "attn_norm", D);
      NEEDF(reg_, w.ffn_norm, P + "ffn_norm", D);
      NEEDF(reg_, w.mod_table, P + "mod_table", 6, D);
      NEEDF(reg_, w.q_norm, P + "q_norm", hd);
      NEEDF(reg_, w.k_norm, P + "k_norm", hd);
      NEEDF(reg_, w.c_q_norm, P + "c_q_norm", hd);
      SA_TRY(need_w5(P + "wqkv", 3 * D, D, w.wqkv));
      SA_TRY(need_w5(P + "wo", D, D, w.wo));
      SA_TRY(need_w5(P + "c_wq", D, D, w.c_wq));
      NEEDW(reg_, AT, w.c_wo.w, P + "c_wo", D, D);
      SA_TRY(need_w5(P + "w13", 2 * F, D, w.w13));
      SA_TRY(need_w5(P + "w2", D, F, w.w2));
      if (!bf16_) {   // SAMAUDIO_OPT_X3_CLASSES: optional split copies, checked when a class is switched on / at the end of finalize
        const struct { const char* leaf; int N, K; LinW& w; } x3w[6] = {{"wqkv", 3 * D, D, w.wqkv}, {"wo", D, D, w.wo},
                                                                        {"c_wq", D, D, w.c_wq},     {"c_wo", D, D, w.c_wo},
                                                                        {"w13", 2 * F, D, w.w13},   {"w2", D, F, w.w2}};
        for (const auto& t : x3w) reg_.twin(P + t.leaf + ".x3", t.N, 3L * t.K, t.w);
      }
    }
    NEEDF(reg_, g_.final_table, "final_table", 2, D);
    NEEDF(reg_, g_.final_norm, "final_norm", D);
    NEEDW(reg_, AT, g_.w_out, "w_out", C2, D);
    NEEDF(reg_, g_.gn1_w, "patch1.gn_w", D);
    NEEDF(reg_, g_.gn1_b, "patch1.gn_b", D);
    NEEDW(reg_, AT, g_.pw1.w, "patch1.w", D, 3 * D);
    NEEDF(reg_, g_.pb1, "patch1.b", D);
    NEEDF(reg_, g_.gn2_w, "patch2.gn_w", D);
    NEEDF(reg_, g_.gn2_b, "patch2.gn_b", D);
    NEEDW(reg_, AT, g_.pw2.w, "patch2.w", D, 3 * D);
    NEEDF(reg_, g_.pb2, "patch2.b", D);
    NEEDW(reg_, AT, g_.y_w13, "y_w13", 2 * D, D);
    NEEDW(reg_, AT, g_.y_w2, "y_w2", D, D);
    NEEDW(reg_, AT, g_.t_w13, "t_w13", 2 * D, cfg_.freq_dim);
    NEEDW(reg_, AT, g_.t_w2, "t_w2", D, D);
    NEEDW(reg_, AT, g_.tb_w, "tb_w", 6 * D, D);
    NEEDF(reg_, g_.tb_b, "tb_b", 6 * D);
    NEEDF(reg_, g_.t_freqs, "t_freqs", cfg_.freq_dim / 2);
    NEEDF(reg_, g_.mem_inv_freq, "mem_inv_freq", D / 2);
    NEEDF(reg_, g_.rope_cos, "rope_cos", cfg_.max_positions, hd / 2);
    NEEDF(reg_, g_.rope_sin, "rope_sin", cfg_.max_positions, hd / 2);
    NEEDW(reg_, AT, g_.proj_wy, "proj_wy", D, C2);
    NEEDW(reg_, AT, g_.proj_wf, "proj_wf", D, C2);
    NEEDF(reg_, g_.proj_b, "proj_b", D);
    NEEDW(reg_, AT, g_.mem_w, "mem_w", D, cfg_.text_dim);
    NEEDF(reg_, g_.mem_b, "mem_b", D);
    NEEDW(reg_, AT, g_.vid_w, "vid_w", D, cfg_.video_dim);
    NEEDF(reg_, g_.vid_b, "vid_b", D);
    NEEDF(reg_, g_.vid_ln_w, "vid_ln_w", D);
    NEEDF(reg_, g_.vid_ln_b, "vid_ln_b", D);
    NEEDF(reg_, g_.vid_gate, "vid_gate", 1);
    NEEDF(reg_, g_.anc_emb, "anc_emb", cfg_.anchor_vocab, cfg_.anchor_dim);
    NEEDW(reg_, AT, g_.anc_w, "anc_w", D, cfg_.anchor_dim);
    // cross-attention K|V projections of ALL layers as one operand: the text memory changes with t only through
    // the y-embedder, so one GEMM per evaluation serves the 22 layers (reference transformer.py:382-388, :102-114)
    NEEDW(reg_, AT, g_.c_wkv_all.w, "c_wkv_all", (int64_t)L * 2 * D, D);
    NEEDF(reg_, g_.c_k_norm_all, "c_k_norm_all", L, hd);
    if (bf16_) {  // fp32 copies for SAMAUDIO_OPT_F32_CLASSES: optional, checked when a class is switched on / used
#define OPTF(field, name, ...) g32_.field = (const float*)opt(name ".f32", {__VA_ARGS__})
      OPTF(w_out, "w_out", C2, D);
      OPTF(t_w13, "t_w13", 2 * D, cfg_.freq_dim);
      OPTF(t_w2, "t_w2", D, D);
      OPTF(tb_w, "tb_w", 6 * D, D);
      OPTF(proj_wy, "proj_wy", D, C2);
      OPTF(proj_wf, "proj_wf", D, C2);
      OPTF(mem_w, "mem_w", D, cfg_.text_dim);
      OPTF(vid_w, "vid_w", D, cfg_.video_dim);
      OPTF(anc_w, "anc_w", D, cfg_.anchor_dim);
      OPTF(y_w13, "y_w13", 2 * D, D);
      OPTF(y_w2, "y_w2", D, D);
#undef OPTF
      SA_TRY(check_f32_weights(f32_classes_));
    }
    if (!bf16_) {   // SAMAUDIO_OPT_X3_CLASSES, classes PATCH / CKV: optional split copies
      reg_.twin("patch1.w.x3", D, 9L * D, g_.pw1);
      reg_.twin("patch2.w.x3", D, 9L * D, g_.pw2);
      reg_.twin("c_wkv_all.x3", (int64_t)L * 2 * D, 3L * D, g_.c_wkv_all);
    }
    dit_ready_ = true;   // (check_x3_weights looks at the resolved layers)
    if (const Status s3 = check_x3_weights(x3_classes_); !s3.ok()) { dit_ready_ = false; return s3; }
  } else {
    const int CD = cfg_.codec_dim, CL = cfg_.codec_latent;
    auto res_units = [&](const std::string& P, StageW& s, int C) -> Status {
      for (int j = 0; j < 3; ++j) {
        const std::string R = P + "r" + std::to_string(j) + ".";
        ResUnitW& r = s.r[j];
        r.k1pad = kpad(7 * C, bf16_);
        r.k2pad = kpad(C, bf16_);
        NEEDF(reg_, r.a1, R + "a1", C);
        NEEDW(reg_, AT, r.w1, R + "w1", C, r.k1pad);
        NEEDF(reg_, r.b1, R + "b1", C);
        NEEDF(reg_, r.a2, R + "a2", C);
        NEEDW(reg_, AT, r.w2, R + "w2", C, r.k2pad);
        NEEDF(reg_, r.b2, R + "b2", C);
      }
      return Status{};
    };
    // encoder
    NEEDW(reg_, AT, enc_.in_w, "enc.in.w", cfg_.enc_dim, 64);
    NEEDF(reg_, enc_.in_b, "enc.in.b", cfg_.enc_dim);
    int C = cfg_.enc_dim;
    for (int i = 0; i < 4; ++i) {
      const std::string P = "enc.s" + std::to_string(i) + ".";
      const int s = cfg_.enc_rates[i];
      if (s % 2) return fail(SAMAUDIO_ERR_ARG, "codec strides must be even");
      SA_TRY(res_units(P, enc_.s[i], C));
      NEEDF(reg_, enc_.s[i].a, P + "a", C);
      NEEDW(reg_, AT, enc_.s[i].w, P + "down.w", 2 * C, 2 * s * C);
      NEEDF(reg_, enc_.s[i].b, P + "down.b", 2 * C);
      C *= 2;
    }
    NEEDF(reg_, enc_.out_a, "enc.out.a", C);
    NEEDW(reg_, AT, enc_.out_w, "enc.out.w", CL, 3 * C);
    NEEDF(reg_, enc_.out_b, "enc.out.b", CL);
    NEEDW(reg_, AT, enc_.proj_w, "enc.proj.w", CD, CL);
    NEEDF(reg_, enc_.proj_b, "enc.proj.b", CD);
    enc_ready_ = true;
    // SAMAUDIO_OPT_X3_CLASSES bit CODEC: twins of registered codec weights, keyed by the weight's own pointer.  "<name>.x3": every
    // Cin-block of a row as [W_hi | W_lo | W_hi] (the wide convolutions, gemm_codec_x3); "<name>.fly" (weights.py convert_codec_fly16): the
    // narrow convolutions' weights already split, in the layout the fp32 kernel's on-the-fly multiply reads (common.h GEMM_FLAG_W_FLY16)
    x3_codec_.clear();
    fly_codec_.clear();
    for (const auto& kv : reg_.all()) {
      const std::string& name = kv.first;
      const size_t dot = name.rfind('.');
      const std::string ext = dot == std::string::npos ? "" : name.substr(dot);
      const bool x3t = ext == ".x3";
      if (bf16_ || (!x3t && ext != ".fly") || (name.rfind("enc.", 0) != 0 && name.rfind("dec.", 0) != 0)) continue;
      const TensorRef* base = reg_.find(name.substr(0, dot));
      const TensorRef& t = kv.second;
      if (!base || base->shape.size() != 2 || t.dtype != SAMAUDIO_DT_BF16) continue;
      const int64_t N = base->shape[0], K = base->shape[1];
      if (!x3t) {
        if (t.shape == std::vector<int64_t>{N, 2 * K} && K % 32 == 0) fly_codec_[base->p] = t.p;
      } else if (t.shape.size() == 3 && t.shape[2] % 3 == 0) {
        const int64_t cin = t.shape[2] / 3;
        if (t.shape[0] == N && t.shape[1] * cin == K && cin % 8 == 0) x3_codec_[base->p] = X3CodecW{t.p, (int)cin};
      }
    }
    if (what == 2) return Status{};  // encoder only: the Judge's DACVAEEncoder (reference codec.py:42-78)
    // decoder
    NEEDW(reg_, AT, dec_.proj_w, "dec.proj.w", CL, CD);
    NEEDF(reg_, dec_.proj_b, "dec.proj.b", CL);
    NEEDW(reg_, AT, dec_.in_w, "dec.in.w", cfg_.dec_dim, 7 * CL);
    NEEDF(reg_, dec_.in_b, "dec.in.b", cfg_.dec_dim);
    C = cfg_.dec_dim;
    for (int i = 0; i < 4; ++i) {
      const std::string P = "dec.s" + std::to_string(i) + ".";
      const int s = cfg_.dec_rates[i];
      if (s % 2) return fail(SAMAUDIO_ERR_ARG, "codec strides must be even");
      NEEDF(reg_, dec_.s[i].a, P + "a", C);
      NEEDW(reg_, AT, dec_.s[i].w, P + "up.w", s * (C / 2), 2 * C);
      NEEDF(reg_, dec_.s[i].b, P + "up.b", C / 2);
      C /= 2;
      SA_TRY(res_units(P, dec_.s[i], C));
    }
    dec_.out_kpad = kpad(7 * C, bf16_);
    NEEDF(reg_, dec_.out_a, "dec.out.a", C);
    NEEDW(reg_, AT, dec_.out_w, "dec.out.w", 1, dec_.out_kpad);
    NEEDF(reg_, dec_.out_b, "dec.out.b", 1);
    codec_ready_ = true;
  }
  return Status{};
}

// ---------------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------------
// The folds run for a short text memory on 128-wide heads unless switched off (SAMAUDIO_NO_FOLD): in a 16-bit context the 16-bit fold; in
// an fp32 context whose class CWO (beside any other DiT class) runs on compensated operands, and few enough layers, the fold on those.
Engine::FoldPlan Engine::fold_plan(int Lt) const {
  const int ltp = Lt <= 8 ? 8 : 16;
  const bool all_layers = cfg_.n_layers <= kMaxFoldLayers;
  const bool can = Lt <= 16 && cfg_.dim / cfg_.n_heads == 128 && !std::getenv("SAMAUDIO_NO_FOLD");
  return FoldPlan{ltp, (int)round_up((long)cfg_.n_heads * ltp, 64), can && bf16_, can && x3(SAMAUDIO_CLS_CWO) && all_layers, all_layers};
}

Status Engine::plan_dit(Bump& b, int rows, int T, int Lt, bool assign) {
  const long D = cfg_.dim, F = cfg_.ffn_hidden, C2 = cfg_.latent_channels;
  const long M = (long)rows * T, Mt = (long)rows * Lt, Tp = round_up(T, 64);
  const long nt = rows;  // worst case: one time value per row
  auto f32 = [&](long n) { return (float*)b.take((size_t)n * 4); };
  auto act = [&](long n) { return b.take((size_t)n * esz_); };
  decltype(d_) d{};   // every buffer, in the order the plan carves them
  d.ymid = f32(M * C2); d.aligned = f32(M * D); d.cond = f32(M * D); d.h = f32(M * D);
  // (hp1 also stages the per-clip text projection of a prepare with candidates: B * Lt <= rows * Lt rows of it)
  d.hp1 = f32((M > Mt ? M : Mt) * D); d.text_proj = f32(Mt * D); d.t_emb = f32(nt * D); d.t0 = f32(nt * 6 * D);
  d.tsin = f32(nt * D); d.vtmp = f32(M * D); d.times = f32(4096);
  d.modgs = f32(2L * cfg_.n_layers * nt * 2 * D);   // pre-combined RMSNorm + modulate operands of an evaluation
  d.ybf = act(M * C2); d.xn = act(M * D); d.qkv = act(M * 3 * D);
  d.Q = act((long)rows * Tp * D); d.K = act((long)rows * Tp * D);   // [rows, H, Tp, head_dim]
  d.Vt = act((long)rows * D * Tp);
  d.attn = act(M * D); d.hbf = act(M * D); d.qc = act(M * D); d.ca = act(M * D); d.u = act(M * F);
  d.gnbuf = act((long)rows * (T + 2) * D); d.mem = act(Mt * D); d.yu = act(Mt * D); d.yemb = act(Mt * D);
  d.kvc = act(Mt * 2 * D * cfg_.n_layers); d.temb = act(nt * cfg_.freq_dim); d.tu = act(nt * D); d.tsilu = act(nt * D);
  d.feats = act(M * C2); d.text = act(Mt * cfg_.text_dim); d.video = act(M * cfg_.video_dim);
  d.anch = act(M * cfg_.anchor_dim);
  // fp32 operands of the classes SAMAUDIO_OPT_F32_CLASSES may switch to exact fp32 (16-bit contexts only)
  if (bf16_) {
    d.temb32 = f32(nt * cfg_.freq_dim); d.tu32 = f32(nt * D); d.tsilu32 = f32(nt * D); d.xn32 = f32(M * D);
    d.prep32 = f32(M * (cfg_.video_dim > cfg_.anchor_dim ? cfg_.video_dim : cfg_.anchor_dim));
    d.mem32 = f32(Mt * D); d.yu32 = f32(Mt * D); d.yemb32 = f32(Mt * D);
  }
  // folded cross-attention (fold_plan): probabilities [M, KP] and the per-batch operand U^T [rows][D][KP]
  const FoldPlan fp = fold_plan(Lt);
  const long kp = fp.kp;
  d.probs = fp.fold16 ? act(M * kp) : nullptr;
  // (one slice per layer: the folds of an evaluation run as one launch in front of the layer loop; DBG_FOLD_PER_LAYER - one launch per
  // layer - only ever uses the first slice)
  d.ut = fp.fold16 ? act((long)rows * D * kp * (fp.all_layers ? cfg_.n_layers : 1)) : nullptr;
  // SAMAUDIO_OPT_X3_CLASSES: the split activation operand [lo | hi | hi] of the widest GEMM input (16-bit, 3 K elements per row)
  // (x3a: D-wide operands - the M frame rows, the Mt text rows of class CKV - and the patcher's halo-padded rows; x3u: the SwiGLU
  // hidden, written by the w13 launch while it reads x3a)
  const bool x3g = !bf16_ && (x3_classes_ & ~(SAMAUDIO_X3_ATTENTION | SAMAUDIO_CLS_CODEC));
  const long x3a_rows = (long)rows * (T + 2) > Mt ? (long)rows * (T + 2) : Mt;
  d.x3a_bytes = x3g ? (size_t)x3a_rows * 3 * (size_t)D * 2 : 0;
  d.x3a = x3g ? b.take(d.x3a_bytes) : nullptr;
  d.x3u_bytes = x3g ? (size_t)M * 3 * (size_t)F * 2 : 0;
  d.x3u = x3g ? b.take(d.x3u_bytes) : nullptr;
  // folded cross-attention on compensated operands: probabilities [M][3 kp] and the per-batch operands of all layers [L][rows][D][3 kp]
  d.x3p = fp.fold3 ? b.take((size_t)M * 3 * kp * 2) : nullptr;
  d.ut3 = fp.fold3 ? b.take((size_t)rows * D * 3 * kp * 2 * cfg_.n_layers) : nullptr;
  d.pad_mask = (unsigned char*)b.take((size_t)M);
  d.text_mask = (unsigned char*)b.take((size_t)Mt);
  d.gn_part = (double*)b.take((size_t)rows * 64 * 2 * 8);
  if (assign) d_ = d;
  return Status{};
}

static long codec_hop(const samaudio_config& c) { return (long)c.enc_rates[0] * c.enc_rates[1] * c.enc_rates[2] * c.enc_rates[3]; }

// per-item element counts of the codec stage buffers (see codec_encode / codec_decode)
static void codec_stage_dims(const samaudio_config& c, int64_t samples, long encT[5], int encC[5], long decT[5],
                             int decC[5]) {
  long T = samples;
  int C = c.enc_dim;
  for (int i = 0; i < 5; ++i) {
    encT[i] = T; encC[i] = C;
    if (i < 4) { T /= c.enc_rates[i]; C *= 2; }
  }
  T = samples / codec_hop(c);
  C = c.dec_dim;
  for (int i = 0; i < 5; ++i) {
    decT[i] = T; decC[i] = C;
    if (i < 4) { T *= c.dec_rates[i]; C /= 2; }
  }
}

struct Engine::SBuf {   // one codec stage: raw fp32 stream, activated copy, a second halo-zeroed buffer of the same shape
  float* raw; void* act; void* tmp;
  long T; int C;
};
struct Engine::CodecBufs {
  void *in8, *eout;   // encode: the waveform as [HALO + S + HALO][8], the latent in front of the projection
  void *lat, *p0;     // decode: the latent, its projection
  SBuf sb[5];
  void* x3; size_t x3_bytes;   // split scratch of gemm_codec_x3 (null: no twin can run)
};

// The linear model the codec workspace is sized by: kCodecFixed + n * per_item, per_item = the bytes of one item's buffers plus, per
// stage and for the split scratch, slack for Bump's 256-byte alignment of the takes (the fixed part covers the remaining ones).
constexpr size_t kCodecFixed = 1 << 16, kCodecStageSlack = 1024, kCodecX3Slack = 256;

size_t Engine::plan_codec(Bump& b, bool decode, int n, int64_t S, CodecBufs* out) const {
  long encT[5], decT[5];
  int encC[5], decC[5];
  codec_stage_dims(cfg_, S, encT, encC, decT, decC);
  const long* T = decode ? decT : encT;
  const int* C = decode ? decC : encC;
  size_t model = 0;
  auto take = [&](size_t item_bytes) { model += (size_t)n * item_bytes; return b.take((size_t)n * item_bytes); };
  auto halo = [](long t, int c) { return (size_t)(t + 2 * HALO) * c; };   // elements of one item's halo-padded [t][c]
  CodecBufs cb{};
  if (decode) { cb.lat = take(halo(T[0], cfg_.codec_dim) * esz_); cb.p0 = take(halo(T[0], cfg_.codec_latent) * esz_); }
  else cb.in8 = take(halo(S, 8) * esz_);
  for (int i = 0; i < 5; ++i) {
    const size_t e = halo(T[i], C[i]);
    cb.sb[i] = SBuf{(float*)take(e * 4), take(e * esz_), take(e * esz_), T[i], C[i]};
    model += (size_t)n * kCodecStageSlack;
  }
  if (!decode) cb.eout = take(halo(T[4], cfg_.codec_latent) * esz_);
  // the split activation operand of the widest launch - of either direction - that can run as a compensated 16-bit launch
  // (gemm_codec_x3): the whole halo buffer it reads, 3 x 16 bits per element; nothing unless the option and the twins are there
  size_t x3_item = 0;
  if (x3(SAMAUDIO_CLS_CODEC) && !x3_codec_.empty()) {
    auto see = [&](long t, int c) { x3_item = std::max(x3_item, halo(t, c) * 6 + kCodecX3Slack); };
    for (int i = 0; i < 5; ++i) {
      if (2 * encC[i] >= 256) see(encT[i], encC[i]);   // (the strided convolution out of stage i has 2 C outputs)
      if (decC[i] >= 256) see(decT[i], decC[i]);
    }
    see(decT[0], cfg_.codec_dim);
    see(decT[0], cfg_.codec_latent);
    cb.x3_bytes = (size_t)n * x3_item;
    cb.x3 = take(x3_item);
  }
  if (out) *out = cb;
  return model;
}

size_t Engine::codec_per_item(int64_t samples) const {
  Bump enc, dec;
  return std::max(plan_codec(enc, false, 1, samples, nullptr), plan_codec(dec, true, 1, samples, nullptr));
}

size_t Engine::codec_bytes(int items, int64_t samples) const { return items <= 0 ? 0 : (size_t)items * codec_per_item(samples) + kCodecFixed; }

// A workspace holds (bytes - kCodecFixed) / per_item waveforms per pass: dividing by codec_bytes(1) would turn a workspace sized for
// exactly n of them into passes of n - 1 and 1 (and the stray single-waveform pass runs at a fraction of the rate)
int Engine::codec_chunk(int items, int64_t samples, bool pairs) const {
  const size_t per_item = codec_per_item(samples);
  int chunk = ws_ && ws_bytes_ > kCodecFixed ? (int)((ws_bytes_ - kCodecFixed) / (per_item ? per_item : 1)) : 0;
  if (chunk > items) chunk = items;
  if (pairs && chunk > 1) chunk &= ~1;   // a pass holds whole (target, residual) pairs
  return pairs && chunk < 2 ? 0 : chunk;
}

size_t Engine::workspace_bytes(int rows, int frames, int text_len, int codec_items, int64_t samples) {
  size_t dit = 0;
  if (rows > 0) {
    Bump b;
    plan_dit(b, rows, frames, text_len < 1 ? 1 : text_len, false);
    dit = b.used() + 4096;
  }
  size_t codec = codec_bytes(codec_items, samples);
  return dit > codec ? dit : codec;
}

Status Engine::set_workspace(void* p, size_t bytes) {
  if (!p || (reinterpret_cast<uintptr_t>(p) & 255)) return fail(SAMAUDIO_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  ws_ = (char*)p;
  ws_bytes_ = bytes;
  prepared_ = false;
  return Status{};
}

// algorithmic bytes of one GEMM / implicit-convolution launch: every operand, output and residual element once
static double gemm_alg_bytes(const GemmParams& p, size_t esz) {
  const double rows = (double)p.M * p.nbatch;
  const double n_out = p.swiglu ? p.N / 2 : p.N;
  const long a_row = p.lda > 0 && p.lda < p.K ? p.lda : p.K;  // implicit convolutions re-read a row once per tap
  double b = rows * (double)a_row * esz + (double)p.N * p.K * esz * (p.w_bstride ? p.nbatch : 1);
  if (p.out_f32) b += rows * n_out * 4;
  if (p.out_act) b += rows * n_out * esz;
  if (p.res) b += (p.res_ld ? rows : 1.0) * n_out * 4;
  return b;
}

Status Engine::check_f32_weights(int classes) const {
  const struct { int cls; const float* w; const char* name; } need[] = {
      {SAMAUDIO_CLS_OUT, g32_.w_out, "w_out"},       {SAMAUDIO_CLS_TIME, g32_.t_w13, "t_w13"},   {SAMAUDIO_CLS_TIME, g32_.t_w2, "t_w2"},
      {SAMAUDIO_CLS_TIME, g32_.tb_w, "tb_w"},        {SAMAUDIO_CLS_IN, g32_.proj_wy, "proj_wy"}, {SAMAUDIO_CLS_PREP, g32_.proj_wf, "proj_wf"},
      {SAMAUDIO_CLS_PREP, g32_.mem_w, "mem_w"},      {SAMAUDIO_CLS_PREP, g32_.vid_w, "vid_w"},   {SAMAUDIO_CLS_PREP, g32_.anc_w, "anc_w"},
      {SAMAUDIO_CLS_YEMB, g32_.y_w13, "y_w13"},      {SAMAUDIO_CLS_YEMB, g32_.y_w2, "y_w2"}};
  for (const auto& n : need)
    if ((classes & n.cls) && !n.w)
      return fail(SAMAUDIO_ERR_WEIGHT, std::string("SAMAUDIO_OPT_F32_CLASSES: the fp32 operand copy '") + n.name +
                                           ".f32' of a class that is switched to fp32 is not registered");
  return Status{};
}

Status Engine::check_x3_weights(int classes) const {
  if (!classes) return Status{};
  if ((classes & SAMAUDIO_CLS_PATCH) && !(g_.pw1.w3 && g_.pw2.w3))
    return fail(SAMAUDIO_ERR_WEIGHT, "SAMAUDIO_OPT_X3_CLASSES: the split weights 'patch1.w.x3' / 'patch2.w.x3' (16-bit, [D, 9D] or [9D/64, D, 64]) are not registered");
  if ((classes & SAMAUDIO_CLS_CKV) && !g_.c_wkv_all.w3)
    return fail(SAMAUDIO_ERR_WEIGHT, "SAMAUDIO_OPT_X3_CLASSES: the split weight 'c_wkv_all.x3' (16-bit, [L*2D, 3D] or [3D/64, L*2D, 64]) is not registered");
  for (size_t i = 0; i < layers_.size(); ++i) {
    const LayerW& w = layers_[i];
    const struct { int cls; const void* p; const char* leaf; } need[6] = {
        {SAMAUDIO_CLS_QKV, w.wqkv.w3, "wqkv"}, {SAMAUDIO_CLS_WO, w.wo.w3, "wo"},    {SAMAUDIO_CLS_CWQ, w.c_wq.w3, "c_wq"},
        {SAMAUDIO_CLS_CWO, w.c_wo.w3, "c_wo"}, {SAMAUDIO_CLS_W13, w.w13.w3, "w13"}, {SAMAUDIO_CLS_W2, w.w2.w3, "w2"}};
    for (const auto& n : need)
      if ((classes & n.cls) && !n.p)
        return fail(SAMAUDIO_ERR_WEIGHT, "SAMAUDIO_OPT_X3_CLASSES: the split weight 'L" + std::to_string(i) + "." + n.leaf +
                                             ".x3' (16-bit, [N, 3K] or [3K/64, N, 64]) of a class that is switched on is not registered");
  }
  return Status{};
}

Status Engine::set_option(int option, int value) {
  if (option == SAMAUDIO_OPT_TAIL_SPLIT) {
    tail_split_ = value != 0;
    return Status{};
  }
  if (option == SAMAUDIO_OPT_F32_CLASSES) {
    if (value && !bf16_) return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_F32_CLASSES applies to 16-bit contexts (an fp32 context is exact already)");
    if (value & ~SAMAUDIO_CLS_F32_CAPABLE)
      return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_F32_CLASSES: only the classes of SAMAUDIO_CLS_F32_CAPABLE can run in fp32");
    if (dit_ready_) SA_TRY(check_f32_weights(value));   // (before finalize(0): checked there)
    f32_classes_ = value;
    return Status{};
  }
  if (option == SAMAUDIO_OPT_ALT16_CLASSES) {
    if (value && !bf16_) return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_ALT16_CLASSES applies to 16-bit contexts");
    if (value & ~SAMAUDIO_CLS_ALT16_CAPABLE)
      return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_ALT16_CLASSES: only the five big GEMM classes of the DiT layers (qkv, wo, cwq, w13, w2)");
    // (what eval_field needs for these classes: the pre-combined RMSNorm operands - checked here, not at the first evaluation)
    if (value && !(2 * cfg_.n_layers <= kMaxModNorms && cfg_.n_layers > 0 && cfg_.dim <= 256 * 12))
      return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_ALT16_CLASSES (precision 'mixed') supports 1 .. " + std::to_string(kMaxModNorms / 2) +
                                        " layers and dim <= 3072: this config has " + std::to_string(cfg_.n_layers) + " layers, dim " +
                                        std::to_string(cfg_.dim) + " - use precision 'fp16' or 'bf16'");
    alt_classes_ = value;
    return Status{};
  }
  if (option == SAMAUDIO_OPT_PREFETCH_ROWS) {
    if (value && !bf16_) return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_PREFETCH_ROWS applies to 16-bit contexts");
    if (value < 0) return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_PREFETCH_ROWS: a row count (0 = off)");
    prefetch_rows_ = value;
    return Status{};
  }
  if (option == SAMAUDIO_OPT_X3_CLASSES) {
    if (value && bf16_) return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_X3_CLASSES applies to fp32 contexts (compensated 16-bit operands under fp32 storage)");
    if (value & ~SAMAUDIO_CLS_X3_CAPABLE)
      return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_X3_CLASSES: only the six big GEMM classes of the DiT layers (qkv, wo, cwq, cwo, w13, w2), patch, ckv, codec and SAMAUDIO_X3_ATTENTION");
    if (dit_ready_) SA_TRY(check_x3_weights(value));   // (before finalize(0): checked there)
    if (((value & ~(SAMAUDIO_X3_ATTENTION | SAMAUDIO_CLS_CODEC)) != 0) != ((x3_classes_ & ~(SAMAUDIO_X3_ATTENTION | SAMAUDIO_CLS_CODEC)) != 0)) prepared_ = false;   // the scratch operand is part of the workspace plan
    x3_classes_ = value;
    return Status{};
  }
  if (option == SAMAUDIO_OPT_SENTINEL) {
    sentinel_on_ = value != 0;
    return Status{};
  }
  if (option == SAMAUDIO_OPT_QUANT_CLASSES || option == SAMAUDIO_OPT_QUANT_FORMAT) {
    if (value && bf16_) return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_QUANT_*: operand-rounding emulation needs an fp32 context");
    if (option == SAMAUDIO_OPT_QUANT_FORMAT && (value < 0 || value > 2))
      return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_QUANT_FORMAT: 0 (off), 1 (bfloat16) or 2 (fp16)");
    (option == SAMAUDIO_OPT_QUANT_CLASSES ? quant_classes_ : quant_fmt_) = value;
    return Status{};
  }
  return fail(SAMAUDIO_ERR_ARG, "samaudio_set_option: unknown option " + std::to_string(option));
}

Status Engine::sentinel(int slot, const void* x, int fmt, long rows, int cols, long ld, hipStream_t st) {
  if (!sentinel_on_ || !x) return Status{};
  constexpr size_t kFloats = 2 * (SAMAUDIO_SENTINEL_SLOTS + kSentinelPartials);
  if (!sentinel_dev_) {
    sentinel_dev_ = (float*)debug_device_alloc(kFloats * 4);
    if (!sentinel_dev_) return fail(SAMAUDIO_ERR_HIP, "sentinel: device allocation failed");
    SA_HIP(hipMemsetAsync(sentinel_dev_, 0, kFloats * 4, st));
  }
  SA_HIP(launch_sentinel(x, fmt, rows, cols, ld, sentinel_dev_ + 2 * SAMAUDIO_SENTINEL_SLOTS, sentinel_dev_ + 2 * slot, st));
  return Status{};
}

Status Engine::sentinel_read(float* absmax, double* nonfinite, hipStream_t st) {
  for (int i = 0; i < SAMAUDIO_SENTINEL_SLOTS; ++i) { absmax[i] = 0.f; nonfinite[i] = 0.0; }
  if (!sentinel_dev_) return Status{};
  float host[2 * SAMAUDIO_SENTINEL_SLOTS];
  SA_HIP(hipStreamSynchronize(st));
  SA_HIP(hipMemcpy(host, sentinel_dev_, sizeof(host), hipMemcpyDeviceToHost));
  SA_HIP(hipMemsetAsync(sentinel_dev_, 0, sizeof(host), st));
  for (int i = 0; i < SAMAUDIO_SENTINEL_SLOTS; ++i) { absmax[i] = host[2 * i]; nonfinite[i] = host[2 * i + 1]; }
  return Status{};
}

static int cls_slot(int cls) {   // the sentinel slot of a class
  int bit = 0;
  while (bit < SAMAUDIO_CLS_COUNT - 1 && !(cls & (1 << bit))) ++bit;
  return bit;
}

// the tag and flags a launch of gemm() runs with (the OUT_SPLIT3 dry run of eval_field asks gemm_check about them)
GemmParams Engine::launch_params(const GemmParams& p_in, int cls, GemmKind kind) const {
  // codec launches run under their own kernel symbols; an x3 launch on K-concatenated split operands shares operand tiles wherever it
  // qualifies (host.h x3_share); X3Block (the convolutions: every Cin-block of K' is its own [hi | lo | hi]) never does
  return gemm_launch_params(p_in, phase_ == Phase::Codec ? 1 : 0, tail_split_, alt16(cls) && kind != GemmKind::F32,
                            kind == GemmKind::X3 ? cls : -1);
}

Status Engine::gemm(const GemmParams& p, hipStream_t st, double alg_flops, int cls, GemmKind kind) {
  SA_TRY(launch(launch_params(p, cls, kind), st, alg_flops, cls, kind));
  return scan_out(p, cls, kind, st);
}

// the 16-bit output of a GEMM launch, scanned into its class's slot (outputs with a window mask - transposed convolutions - have
// rows the launch does not write, x3 launches fp32 outputs: skipped)
Status Engine::scan_out(const GemmParams& p, int cls, GemmKind kind, hipStream_t st) {
  if (!sentinel_on_ || !p.out_act || p.c_ld_rel || kind == GemmKind::X3 || kind == GemmKind::X3Block) return Status{};
  const int fmt = (kind == GemmKind::F32 || !bf16_) ? 0 : ((p.flags & GEMM_FLAG_OUT_ALT) ? 2 : 1);
  const int n_out = p.swiglu ? p.N / 2 : p.N;
  for (int b = 0; b < p.nbatch; ++b) {
    const size_t esz = fmt == 0 ? 4 : 2;
    const char* base = (const char*)p.out_act + ((size_t)p.act_off + (size_t)b * p.act_bstride) * esz;
    SA_TRY(sentinel(cls_slot(cls), base, fmt, p.M, n_out, p.act_ld, st));
  }
  return Status{};
}

const Engine::X3CodecW* Engine::codec_x3_twin(const GemmParams& p) const {
  if (!x3_codec_scratch_ || !x3(SAMAUDIO_CLS_CODEC)) return nullptr;
  const auto it = x3_codec_.find(p.W);
  if (it == x3_codec_.end()) return nullptr;
  return codec_x3_eligible(p, it->second.cin, x3_codec_scratch_bytes_) ? &it->second : nullptr;
}

Status Engine::codec_gemm(const GemmParams& p_in, hipStream_t st, double alg_flops) {
  if (const X3CodecW* w3 = codec_x3_twin(p_in)) {
    SA_TRY(gemm_codec_x3(p_in, *w3, st, alg_flops));
  } else {
    GemmParams p = launch_params(p_in, SAMAUDIO_CLS_CODEC, GemmKind::Native);
    if (x3(SAMAUDIO_CLS_CODEC)) {   // (fp32 contexts): the convolution multiplies on split operands, split in registers (gemm.hip)
      const auto it = fly_codec_.find(p.W);
      codec_fly_operands(p, it != fly_codec_.end() ? it->second : nullptr);
    }
    SA_TRY(launch(p, st, alg_flops, SAMAUDIO_CLS_CODEC, GemmKind::Native));
  }
  return scan_out(p_in, SAMAUDIO_CLS_CODEC, GemmKind::Native, st);
}

Status Engine::launch(GemmParams p, hipStream_t st, double alg_flops, int cls, GemmKind kind) {
  const bool x3m = kind == GemmKind::X3 || kind == GemmKind::X3Block;
  const bool is16 = bf16_ || x3m;   // the launch's operand format (an x3 launch: 16-bit operands inside an fp32 context)
  const double flops = alg_flops >= 0 ? alg_flops : 2.0 * p.M * (double)p.N * p.K * p.nbatch;
  if (kind == GemmKind::F32) {  // a class of SAMAUDIO_OPT_F32_CLASSES: exact-fp32 kernel inside a 16-bit context
    if (!p.W) return fail(SAMAUDIO_ERR_WEIGHT, "SAMAUDIO_OPT_F32_CLASSES: the class's \"<name>.f32\" weight copy is not registered");
    if (const char* why = gemm_check(p, false)) return fail(SAMAUDIO_ERR_ARG, why);
    return op(gemm_variant_name(gemm_variant(p, false), false), gemm_alg_bytes(p, 4), flops, st,
              [&] { return launch_gemm(p, false, st); });
  }
  if (!is16 && quant_fmt_ && (quant_classes_ & cls)) p.flags |= (quant_fmt_ << GEMM_FLAG_QUANT_A_SHIFT) | (quant_fmt_ << GEMM_FLAG_QUANT_W_SHIFT);
  if (const char* why = gemm_check(p, is16)) return fail(SAMAUDIO_ERR_ARG, why);
  if (!prof_on_) {
    SA_HIP(launch_gemm(p, is16, st));
    return Status{};
  }
  const double bytes = gemm_alg_bytes(p, is16 ? 2 : 4);
  const int full = gemm_tail_split(p, is16);
  const long tiles = (long)((p.M + 255) / 256) * ((p.N + 255) / 256) * p.nbatch;
  for (int part = 0; part < (full ? 2 : 1); ++part) {
    // a split launch (gemm.hip gemm_tail_split) is two kernels: each gets its own record, flops / bytes by tile share
    const double share = !full ? 1.0 : (part == 0 ? (double)full / tiles : 1.0 - (double)full / tiles);
    ProfRec r;
    // implicit convolutions (kc < K) run the 8-phase kernels under their own instantiation (gemm8_kernel<true>): own record
    const int variant = gemm_variant(p, is16);
    const char* conv = gemm_is_8phase(variant) && p.kc < p.K ? "_conv" : "";
    r.key = std::string(phase_name()) + "/" + (part ? kGemm8sTailName : gemm_variant_name(variant, is16)) + conv + (x3m ? "_x3" : "");
    if (static const bool by_class = std::getenv("SAMAUDIO_PROF_BY_CLASS") != nullptr; by_class) {   // diagnosis: one record per GEMM class
      int bit = 0;
      while (bit < SAMAUDIO_CLS_COUNT && !(cls & (1 << bit))) ++bit;
      r.key += "#" + std::to_string(bit);
    }
    r.flops = flops * share;
    r.bytes = bytes * share;
    SA_TRY(prof_event(&r.e0));
    SA_TRY(prof_event(&r.e1));
    SA_HIP(hipEventRecord(r.e0, st));
    if (full) SA_HIP(launch_gemm_part(p, is16, part, st));
    else SA_HIP(launch_gemm(p, is16, st));
    SA_HIP(hipEventRecord(r.e1, st));
    prof_.push_back(r);
  }
  return Status{};
}

Status Engine::linear(GemmParams p, const LinW& w, int cls, hipStream_t st, const void* presplit, bool ffn_wide) {
  if (!x3(cls)) {
    p.W = w.w;
    if (w.ktm) p.flags |= GEMM_FLAG_W_KTM;
    return gemm(p, st, -1.0, cls);
  }
  if (!w.w3 || !d_.x3a) return fail(SAMAUDIO_ERR_STATE, "SAMAUDIO_OPT_X3_CLASSES: split weight or scratch operand missing (set the option before samaudio_prepare)");
  if (!x3_whole_k(p) || p.nbatch != 1 || p.a_off)
    return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_X3_CLASSES: plain single-batch launches with one output only");
  const int K = p.K;
  if (!presplit) {   // split the fp32 operand here: into x3a (D-wide rows), or - w2's F-wide hidden - into x3u
    void* const dst = ffn_wide ? d_.x3u : d_.x3a;
    SA_TRY(x3_fits(dst, ffn_wide ? d_.x3u_bytes : d_.x3a_bytes, p.M, K, "", "the split operand does not fit the scratch the workspace plan holds"));
    // algorithmic bytes of the split: the fp32 row in, three 16-bit copies out
    SA_TRY(op("split3", (double)p.M * K * (4 + 6), 0, st, [&] { return launch_split3((const float*)p.A, p.lda, dst, p.M, K, st); }));
    presplit = dst;
  }
  x3_operands(p, presplit, w);
  return gemm(p, st, 2.0 * p.M * (double)p.N * K, cls, GemmKind::X3);   // flops as the reference counts them: one product over K
}

Status Engine::gemm_codec_x3(const GemmParams& p_in, const X3CodecW& w, hipStream_t st, double alg_flops) {
  // the geometry - the split, the restated launch, X3 / X3Block, the activation pass - is host.h's (codec_x3_*): here the launches
  const int c = w.cin;
  const long rows = codec_x3_split_rows(p_in, c);
  SA_TRY(op("split3", (double)rows * c * (4 + 6), 0, st, [&] { return launch_split3((const float*)p_in.A, c, x3_codec_scratch_, rows, c, st); }));
  const double flops = alg_flops >= 0 ? alg_flops : 2.0 * p_in.M * (double)p_in.N * p_in.K * p_in.nbatch;
  SA_TRY(gemm(codec_x3_launch(p_in, x3_codec_scratch_, w.w), st, flops, SAMAUDIO_CLS_CODEC,
              codec_x3_whole_k(p_in, c) ? GemmKind::X3 : GemmKind::X3Block));
  const CodecActPass a = codec_x3_act(p_in);
  if (!a.run) return Status{};
  if (!a.aligned) return fail(SAMAUDIO_ERR_ARG, "gemm_codec_x3: window start is not a whole channel row");
  return op("codec_act", (double)a.count * a.items * 8, 0, st, [&] {
    return launch_act_flat(a.in, a.in_bstride, a.out, a.out_bstride, a.items, a.count, a.chan, a.act, a.alpha, st);
  });
}

// One DAC residual unit: k7 convolution `p` (Snake'd bf16 intermediate) followed by the k1 convolution `q` on it
// (+ fp32 residual, Snake'd bf16 copy out).  `cur` = the unit's input activation, `alt` = a second halo-zeroed buffer of
// the same shape.  Large bf16 launches run as ONE kernel (gemm2.hip resunit_kernel: the intermediate stays in LDS) that
// writes its activation to `alt` - it must not overwrite rows neighbouring tiles still read - and the buffers swap roles;
// everything else runs as the two launches with `alt` as the intermediate.  Both forms are bitwise identical.
Status Engine::res_unit(GemmParams p, GemmParams q, void*& cur, void*& alt, double flops7, double flops1, hipStream_t st) {
  p.out_act = alt;
  q.A = alt;
  q.out_act = cur;
  GemmParams fp = p, fq = q;
  fq.out_act = alt;
  fp.tag = fq.tag = phase_ == Phase::Codec ? 1 : 0;
  const bool covered = p.N == 64 || p.N == 96 || p.N == 128 || p.N == 192;
  // fused for all four channel counts: since the residual-unit kernels issue their direct-to-LDS loads as inline assembly
  // (gemm2.hip dma16a) the fused form is the faster one everywhere (profiles/r3_call12/op_bench.log, 8 waveforms, fused vs
  // two launches: C = 64 923 vs 1193 us, C = 96 1697 vs 2269, C = 128 1353 vs 1391, C = 192 2515 vs 2784)
  const bool fuse = bf16_ && covered && !debug_flag(DBG_RESUNIT_TWO_LAUNCHES) && resunit_ok(fp, fq) &&
                    ((long)((p.M + 255) / 256) * p.nbatch >= 256 || debug_flag(DBG_RESUNIT_FUSE_ALWAYS));
  if (!fuse) {
    SA_TRY(codec_gemm(p, st, flops7));
    return codec_gemm(q, st, flops1);
  }
  if (const char* why = gemm_check(fp, bf16_)) return fail(SAMAUDIO_ERR_ARG, why);
  if (const char* why = gemm_check(fq, bf16_)) return fail(SAMAUDIO_ERR_ARG, why);
  const double inter = (double)p.M * p.N * p.nbatch * esz_;   // the intermediate: neither written nor read
  SA_TRY(op("resunit_bf16", gemm_alg_bytes(fp, esz_) + gemm_alg_bytes(fq, esz_) - 2 * inter, flops7 + flops1, st,
            [&] { return launch_resunit(fp, fq, st); }));
  SA_TRY(scan_out(fq, SAMAUDIO_CLS_CODEC, GemmKind::Native, st));   // the fused unit's 16-bit output (halo layout: the rows the launch writes)
  std::swap(cur, alt);
  return Status{};
}

template <class F>
Status Engine::op(const char* name, double alg_bytes, double alg_flops, hipStream_t st, F&& launch) {
  if (!prof_on_) {
    SA_HIP(launch());
    return Status{};
  }
  ProfRec r;
  r.key = std::string(phase_name()) + "/" + name;
  r.flops = alg_flops;
  r.bytes = alg_bytes;
  SA_TRY(prof_event(&r.e0));
  SA_TRY(prof_event(&r.e1));
  SA_HIP(hipEventRecord(r.e0, st));
  SA_HIP(launch());
  SA_HIP(hipEventRecord(r.e1, st));
  prof_.push_back(r);
  return Status{};
}

Status Engine::prof_event(hipEvent_t* e) {
  if (ev_used_ == ev_pool_.size()) {
    hipEvent_t ev;
    SA_HIP(hipEventCreate(&ev));
    ev_pool_.push_back(ev);
  }
  *e = ev_pool_[ev_used_++];
  return Status{};
}

Status Engine::profile_begin() {
  prof_.clear();
  ev_used_ = 0;
  prof_on_ = true;
  return Status{};
}

Status Engine::profile_end(std::vector<KernelStat>& out) {
  prof_on_ = false;
  out.clear();
  std::map<std::string, size_t> index;
  for (const ProfRec& r : prof_) {
    SA_HIP(hipEventSynchronize(r.e1));
    float ms = 0.f;
    SA_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
    auto it = index.find(r.key);
    if (it == index.end()) {
      it = index.emplace(r.key, out.size()).first;
      out.push_back(KernelStat{});
      out.back().name = r.key;
    }
    KernelStat& k = out[it->second];
    k.launches += 1;
    k.flops += r.flops;
    k.bytes += r.bytes;
    k.ms += ms;
  }
  prof_.clear();
  ev_used_ = 0;
  return Status{};
}

Engine::~Engine() {
  for (hipEvent_t e : ev_pool_) (void)hipEventDestroy(e);
  debug_device_free(sentinel_dev_);
  if (hash_) {   // SAMAUDIO_TRACE_HASH recorder
    HashTrace* h = (HashTrace*)hash_;
    debug_device_free(h->dev);
    delete h;
  }
}

static void out_f32(GemmParams& p, float* o, long ld) { p.out_f32 = o; p.f32_ld = ld; }
static void out_act(GemmParams& p, void* o, long ld, int act = ACT_NONE) { p.out_act = o; p.act_ld = ld; p.act = act; }
static void with_res(GemmParams& p, const float* r, long ld) { p.res = r; p.res_ld = ld; }

// ---------------------------------------------------------------------------------------------------
// conditioning that is constant over the ODE (hoisted out of the 32 evaluations)
// ---------------------------------------------------------------------------------------------------
Status Engine::prepare(int rows, int T, int Lt, const float* feats, const float* text, const uint8_t* text_mask,
                       const float* video, const int64_t* anchor_ids, int n_ids, const int64_t* anchor_alignment,
                       const uint8_t* pad_mask, hipStream_t st, int cand, bool latent_feats) {
  win_next_ = nullptr;   // a successor table (samaudio_set_windows) belongs to the rows it was set for: it never meets a new batch
  win_overlap_ = 0;
  win_groups_ = nullptr;   // and so do the group table and the ownership mask (samaudio_set_window_groups)
  win_owner_ = nullptr;
  win_n_groups_ = 0;
  if (!dit_ready_) return fail(SAMAUDIO_ERR_STATE, "prepare: DiT weights not finalized");
  if (rows <= 0 || T <= 0 || !feats) return fail(SAMAUDIO_ERR_ARG, "prepare: bad shape");
  if (cand < 1 || rows % cand) return fail(SAMAUDIO_ERR_ARG, "prepare: rows must be a multiple of candidates");
  if (T > cfg_.max_positions) return fail(SAMAUDIO_ERR_ARG, "prepare: more frames than RoPE positions");
  if (text && Lt <= 0) return fail(SAMAUDIO_ERR_ARG, "prepare: text_len must be positive");
  if (!text) Lt = 1;
  if (anchor_ids && (!anchor_alignment || n_ids <= 0)) return fail(SAMAUDIO_ERR_ARG, "prepare: anchors incomplete");
  phase_ = Phase::Prep;
  Bump b(ws_, ws_bytes_);
  plan_dit(b, rows, T, Lt, true);
  if (!ws_ || !b.fits())
    return fail(SAMAUDIO_ERR_WORKSPACE, "prepare: workspace too small (" + std::to_string(b.used()) + " bytes needed)");
  rows_ = rows; frames_ = T; text_len_ = Lt; frames_pad_ = (int)round_up(T, 64);
  const int D = cfg_.dim, C2 = cfg_.latent_channels;
  const long M = (long)rows * T, Mt = (long)rows * Lt;
  // the conditioning is computed once per CLIP (B = rows / candidates of them) and then repeated for the clip's candidates: the
  // per-clip results live in buffers the evaluations overwrite anyway (aligned, hp1 - which plan_dit sizes for Lt > T too) until the
  // repeat kernels have read them
  const int B = rows / cand;
  const long Mb = (long)B * T, Mtb = (long)B * Lt;
  float* const cond_b = cand > 1 ? d_.aligned : d_.cond;
  float* const textp_b = cand > 1 ? d_.hp1 : d_.text_proj;

  if (pad_mask && cand > 1) SA_HIP(launch_repeat_rows_u8(pad_mask, d_.pad_mask, B, cand, T, st));
  else if (pad_mask) SA_HIP(hipMemcpyAsync(d_.pad_mask, pad_mask, M, hipMemcpyDeviceToDevice, st));
  else SA_HIP(hipMemsetAsync(d_.pad_mask, 1, M, st));
  if (text && text_mask && cand > 1) SA_HIP(launch_repeat_rows_u8(text_mask, d_.text_mask, B, cand, Lt, st));
  else if (text && text_mask) SA_HIP(hipMemcpyAsync(d_.text_mask, text_mask, Mt, hipMemcpyDeviceToDevice, st));
  else SA_HIP(hipMemsetAsync(d_.text_mask, 1, Mt, st));
  // patcher conv input: halo rows stay zero for the whole solve
  SA_HIP(hipMemsetAsync(d_.gnbuf, 0, (size_t)rows * (T + 2) * D * esz_, st));

  // SAMAUDIO_CLS_PREP in exact fp32 (16-bit contexts): the caller's fp32 tensors are the operands themselves
  const bool pf = f32c(SAMAUDIO_CLS_PREP);
  const int PREP = SAMAUDIO_CLS_PREP;
  const GemmKind pk = f32_if(pf);
  // cond = proj_b + audio_features @ Wf^T                           (model.py:116-125, columns 512..767)
  // latent_feats: audio_features = (z | z) of the codec latent z [Mb, C2 / 2] (model.py:182-184): the K axis of this GEMM is two
  // taps of C2 / 2 channels that read the SAME row (tap stride 0) - the same products in the same order as on the concatenation
  const int fw = latent_feats ? C2 / 2 : C2;   // width of the rows `feats` holds
  if (!pf) SA_HIP(launch_to_act(feats, 0, fw, 0, d_.feats, 0, bf16_, 1, Mb, fw, fw, 0, st));
  {
    GemmParams p = pf ? lin(feats, fw, g32_.proj_wf, Mb, D, C2) : lin(d_.feats, fw, g_.proj_wf, Mb, D, C2);
    if (latent_feats) { p.kc = fw; p.tap_stride = 0; }
    p.bias = g_.proj_b;
    out_f32(p, cond_b, D);
    SA_TRY(gemm(p, st, -1.0, PREP, pk));
  }
  // cond += tanh(g_v) * LayerNorm(conv1x1(video))                   (align.py:41-50; zeros if no video: Q8)
  const void* vid_op = d_.video;
  if (pf && video) vid_op = video;
  else if (pf) { vid_op = d_.prep32; SA_HIP(hipMemsetAsync(d_.prep32, 0, (size_t)Mb * cfg_.video_dim * 4, st)); }
  else if (video) SA_HIP(launch_to_act(video, 0, cfg_.video_dim, 0, d_.video, 0, bf16_, 1, Mb, cfg_.video_dim, cfg_.video_dim, 0, st));
  else SA_HIP(hipMemsetAsync(d_.video, 0, (size_t)Mb * cfg_.video_dim * esz_, st));
  {
    GemmParams p = lin(vid_op, cfg_.video_dim, pf ? (const void*)g32_.vid_w : g_.vid_w, Mb, D, cfg_.video_dim);
    p.bias = g_.vid_b;
    out_f32(p, d_.vtmp, D);
    SA_TRY(gemm(p, st, -1.0, PREP, pk));
    SA_HIP(launch_layernorm_accum(d_.vtmp, g_.vid_ln_w, g_.vid_ln_b, g_.vid_gate, cond_b, (int)Mb, D, 1e-5f, st));
  }
  // cond += tanh(g_a) * proj(Emb[ids.gather(alignment)])            (model.py:54-65; tanh folded into anc_w)
  // folded cross-attention output projection: zero the probability buffer once (its K padding columns stay zero)
  const FoldPlan fp = fold_plan(Lt);   // (as plan_dit sized it above)
  fold3_ = fp.fold3;
  fold_ltp_ = fp.fold16 || fp.fold3 ? fp.ltp : 0;
  fold_kp_ = fold_ltp_ ? fp.kp : 0;
  if (fp.fold16) {
    SA_HIP(hipMemsetAsync(d_.probs, 0, (size_t)M * fold_kp_ * esz_, st));
    // 0 * (K padding of U) must stay 0
    SA_HIP(hipMemsetAsync(d_.ut, 0, (size_t)rows * D * fold_kp_ * esz_ * (fp.all_layers ? cfg_.n_layers : 1), st));
  }
  if (fp.fold3) {   // x3 context: the fold on compensated operands (zero K padding of P and U, once per prepare)
    SA_HIP(hipMemsetAsync(d_.x3p, 0, (size_t)M * 3 * fold_kp_ * 2, st));
    SA_HIP(hipMemsetAsync(d_.ut3, 0, (size_t)rows * D * 3 * fold_kp_ * 2 * cfg_.n_layers, st));
  }
  has_anchor_ = anchor_ids != nullptr;
  if (anchor_ids) {
    SA_HIP(launch_anchor_gather(g_.anc_emb, (const long*)anchor_ids, n_ids, (const long*)anchor_alignment,
                                pf ? (void*)d_.prep32 : d_.anch, pf ? false : bf16_, B, T, cfg_.anchor_dim,
                                cfg_.anchor_vocab, st));
    GemmParams p = pf ? lin(d_.prep32, cfg_.anchor_dim, g32_.anc_w, Mb, D, cfg_.anchor_dim)
                      : lin(d_.anch, cfg_.anchor_dim, g_.anc_w, Mb, D, cfg_.anchor_dim);
    with_res(p, cond_b, D);
    out_f32(p, cond_b, D);
    SA_TRY(gemm(p, st, -1.0, PREP, pk));
  }
  // text_proj = memory_proj(text)                                   (model.py:171)
  if (text) {
    if (!pf) SA_HIP(launch_to_act(text, 0, cfg_.text_dim, 0, d_.text, 0, bf16_, 1, Mtb, cfg_.text_dim, cfg_.text_dim, 0, st));
    GemmParams p = pf ? lin(text, cfg_.text_dim, g32_.mem_w, Mtb, D, cfg_.text_dim)
                      : lin(d_.text, cfg_.text_dim, g_.mem_w, Mtb, D, cfg_.text_dim);
    p.bias = g_.mem_b;
    out_f32(p, textp_b, D);
    SA_TRY(gemm(p, st, -1.0, PREP, pk));
  } else {
    SA_HIP(hipMemsetAsync(textp_b, 0, (size_t)Mtb * D * 4, st));
  }
  if (cand > 1) {   // sample-major repeat of the per-clip conditioning (model.py:193-203)
    SA_HIP(launch_repeat_items_f32(cond_b, d_.cond, B, cand, (long)T * D, st));
    SA_HIP(launch_repeat_items_f32(textp_b, d_.text_proj, B, cand, (long)Lt * D, st));
  }
  prepared_ = true;
  return Status{};
}

// ---------------------------------------------------------------------------------------------------
// one evaluation of the vector field: out = res + alpha * DiT(align(noisy), t)
// ---------------------------------------------------------------------------------------------------
Status Engine::eval_field(const float* noisy, const float* time, int nt, float* out, const float* res, float alpha,
                          hipStream_t st) {
  if (!prepared_) return fail(SAMAUDIO_ERR_STATE, "forward: call samaudio_prepare first");
  if (nt != 1 && nt != rows_) return fail(SAMAUDIO_ERR_ARG, "forward: n_time must be 1 or rows");
  if (win_next_ && !launch_window_blend)
    return fail(SAMAUDIO_ERR_STATE, "forward: windows are set, but this build has no window_blend_kernel");
  const int D = cfg_.dim, F = cfg_.ffn_hidden, C2 = cfg_.latent_channels, H = cfg_.n_heads, T = frames_,
            Lt = text_len_, Tp = frames_pad_, rows = rows_;
  const long M = (long)rows * T, Mt = (long)rows * Lt;
  const float eps = cfg_.norm_eps;
  const int hd = D / H;   // 128 | 64 (finalize)
  const long t6 = nt == 1 ? 0 : 6L * D, t1 = nt == 1 ? 0 : (long)D;
  phase_ = Phase::Dit;
  const double MD = (double)M * D;
  if (hash_on() && !hash_) hash_ = new HashTrace();
  const HashScope hash_scope(hash_on() ? (HashTrace*)hash_ : nullptr, rows);
  hash_stage("noisy", noisy, (size_t)M * C2 * 4, st);

  // aligned = noisy @ Wy^T + cond                                   (model.py:116-125, columns 0..255)
  {
    const bool f = f32c(SAMAUDIO_CLS_IN);   // exact fp32: the ODE state itself is the operand
    if (!f) SA_HIP(launch_to_act(noisy, 0, C2, 0, d_.ybf, 0, bf16_, 1, M, C2, C2, 0, st));
    GemmParams p = f ? lin(noisy, C2, g32_.proj_wy, M, D, C2) : lin(d_.ybf, C2, g_.proj_wy, M, D, C2);
    with_res(p, d_.cond, D);
    out_f32(p, d_.aligned, D);
    SA_TRY(gemm(p, st, -1.0, SAMAUDIO_CLS_IN, f32_if(f)));
  }
  // patcher: (GroupNorm(1) -> SiLU -> conv k3) x 2 + skip           (patcher.py:138-141)
  auto patch_conv = [&](const LinW& w, const float* bias, const float* skip, float* dst) -> Status {
    GemmParams p = lin(d_.gnbuf, D, w.w, T, D, 3 * D);
    p.kc = D; p.tap_stride = D; p.a_off = 0; p.a_bstride = (long)(T + 2) * D; p.nbatch = rows;
    p.bias = bias;
    if (skip) { with_res(p, skip, D); p.res_bstride = (long)T * D; }
    out_f32(p, dst, D);
    p.f32_bstride = (long)T * D;
    if (!x3(SAMAUDIO_CLS_PATCH)) return gemm(p, st, -1.0, SAMAUDIO_CLS_PATCH);
    // compensated operands: every row of the halo-padded GroupNorm output (halo rows are zeros: they split into zeros) becomes
    // [lo | hi | hi], a tap of the convolution then is 3 D contiguous elements against that tap's [W_hi | W_lo | W_hi]
    if (!w.w3 || !d_.x3a) return fail(SAMAUDIO_ERR_STATE, "SAMAUDIO_OPT_X3_CLASSES: patcher split weight or scratch operand missing");
    const long prow = (long)rows * (T + 2);
    SA_TRY(op("split3", (double)prow * D * (4 + 6), 0, st, [&] { return launch_split3((const float*)d_.gnbuf, D, d_.x3a, prow, D, st); }));
    x3_block_operands(p, d_.x3a, w.w3, w.ktm3);   // K' split per tap: a plain walk
    return gemm(p, st, 2.0 * T * (double)D * 3 * D * rows, SAMAUDIO_CLS_PATCH, GemmKind::X3Block);
  };
  trace("cond", d_.cond, (size_t)M * D, false, st);
  trace("aligned", d_.aligned, (size_t)M * D, false, st);
  SA_TRY(op("groupnorm_silu", MD * (4 + esz_), 0, st, [&] {
    return launch_groupnorm_silu(d_.aligned, g_.gn1_w, g_.gn1_b, d_.gn_part, d_.gnbuf, bf16_, rows, T, D, 1, 1e-5f, st);
  }));
  SA_TRY(patch_conv(g_.pw1, g_.pb1, nullptr, d_.hp1));
  SA_TRY(op("groupnorm_silu", MD * (4 + esz_), 0, st, [&] {
    return launch_groupnorm_silu(d_.hp1, g_.gn2_w, g_.gn2_b, d_.gn_part, d_.gnbuf, bf16_, rows, T, D, 1, 1e-5f, st);
  }));
  SA_TRY(patch_conv(g_.pw2, g_.pb2, d_.aligned, d_.h));

  // timestep embeddings                                             (transformer.py:490-493, model.py:170)
  {
    // one row per time value: in exact fp32 these three GEMMs cost nothing, and their rounding would reach the shift /
    // scale / gate of every row of every layer coherently
    const bool f = f32c(SAMAUDIO_CLS_TIME);
    const int TIME = SAMAUDIO_CLS_TIME;
    void *temb = f ? (void*)d_.temb32 : d_.temb, *tu = f ? (void*)d_.tu32 : d_.tu, *tsilu = f ? (void*)d_.tsilu32 : d_.tsilu;
    SA_HIP(launch_time_features(time, nt, g_.t_freqs, cfg_.freq_dim, g_.mem_inv_freq, D, temb, d_.tsin, f ? false : bf16_, st));
    GemmParams p = lin(temb, cfg_.freq_dim, f ? (const void*)g32_.t_w13 : g_.t_w13, nt, 2 * D, cfg_.freq_dim);
    p.swiglu = 1;
    out_act(p, tu, D);
    SA_TRY(gemm(p, st, -1.0, TIME, f32_if(f)));
    p = lin(tu, D, f ? (const void*)g32_.t_w2 : g_.t_w2, nt, D, D);
    out_f32(p, d_.t_emb, D);
    out_act(p, tsilu, D, ACT_SILU);
    SA_TRY(gemm(p, st, -1.0, TIME, f32_if(f)));
    p = lin(tsilu, D, f ? (const void*)g32_.tb_w : g_.tb_w, nt, 6 * D, D);
    p.bias = g_.tb_b;
    out_f32(p, d_.t0, 6L * D);
    SA_TRY(gemm(p, st, -1.0, TIME, f32_if(f)));
  }
  // RMSNorm + modulate operands of this evaluation, pre-combined for every layer's two norms (kernels.hip mod_tables)
  const bool mod_gs = 2 * cfg_.n_layers <= kMaxModNorms && cfg_.n_layers > 0 && D <= 256 * 12;
  if (alt_classes_ && bf16_ && !mod_gs)
    return fail(SAMAUDIO_ERR_ARG, "SAMAUDIO_OPT_ALT16_CLASSES: the mixed mode needs the pre-combined RMSNorm operands (<= 48 layers, D <= 3072)");
  const long gs_ld = nt == 1 ? 0 : 2L * D;
  if (mod_gs) {
    ModTables mt;
    for (int l = 0; l < cfg_.n_layers; ++l)
      for (int k = 0; k < 2; ++k) {
        const int n = 2 * l + k;
        mt.w[n] = k ? layers_[l].ffn_norm : layers_[l].attn_norm;
        mt.shift_tab[n] = layers_[l].mod_table + (k ? 3 : 0) * D;
        mt.scale_tab[n] = layers_[l].mod_table + (k ? 4 : 1) * D;
        mt.shift_off[n] = (k ? 3 : 0) * D;
        mt.scale_off[n] = (k ? 4 : 1) * D;
      }
    for (int n = 2 * cfg_.n_layers; n < kMaxModNorms; ++n) {
      mt.w[n] = mt.shift_tab[n] = mt.scale_tab[n] = nullptr;
      mt.shift_off[n] = mt.scale_off[n] = 0;
    }
    SA_TRY(op("mod_tables", 2.0 * cfg_.n_layers * (5.0 + 2.0 * nt) * D * 4, 0, st, [&] {
      return launch_mod_tables(mt, 2 * cfg_.n_layers, d_.t0, t6, nt, d_.modgs, D, st);
    }));
  }
  // memory = memory_proj(text) + sincos(t); y = y_embedder(memory)  (model.py:170-172, transformer.py:495)
  {
    const bool f = f32c(SAMAUDIO_CLS_YEMB);
    const int YEMB = SAMAUDIO_CLS_YEMB;
    void *mem = f ? (void*)d_.mem32 : d_.mem, *yu = f ? (void*)d_.yu32 : d_.yu;
    SA_HIP(launch_add_rowvec(d_.text_proj, d_.tsin, t1, mem, f ? false : bf16_, (int)Mt, D, Lt, st));
    GemmParams p = lin(mem, D, f ? (const void*)g32_.y_w13 : g_.y_w13, Mt, 2 * D, D);
    p.swiglu = 1;
    out_act(p, yu, D);
    SA_TRY(gemm(p, st, -1.0, YEMB, f32_if(f)));
    p = lin(yu, D, f ? (const void*)g32_.y_w2 : g_.y_w2, Mt, D, D);
    if (f) {  // the K | V projections read the 16-bit copy
      out_f32(p, d_.yemb32, D);
      SA_TRY(gemm(p, st, -1.0, YEMB, GemmKind::F32));
      SA_HIP(launch_to_act(d_.yemb32, 0, D, 0, d_.yemb, 0, true, 1, Mt, D, D, 0, st));
    } else {
      out_act(p, d_.yemb, D);
      SA_TRY(gemm(p, st, -1.0, YEMB));
    }
  }

  trace("patcher out h", d_.h, (size_t)M * D, false, st);
  trace("t0", d_.t0, (size_t)nt * 6 * D, false, st);
  trace("yemb", d_.yemb, (size_t)Mt * D, bf16_, st);
  const long kv_ld = 2L * D * cfg_.n_layers;
  if (cfg_.n_layers > 0) {  // cross-attention keys / values of every layer (k-normed), [Mt, L*2D]
    GemmParams p = lin(d_.yemb, D, nullptr, Mt, (int)kv_ld, D);   // (W: linear sets it from the record, here and below)
    out_act(p, d_.kvc, kv_ld);
    SA_TRY(linear(p, g_.c_wkv_all, SAMAUDIO_CLS_CKV, st));
    SA_HIP(launch_headnorm_layers(d_.kvc, g_.c_k_norm_all, bf16_, (int)Mt, cfg_.n_layers, H, eps, st, hd));
  }
  trace("kvc", d_.kvc, (size_t)Mt * kv_ld, bf16_, st);
  // folded cross-attention: U_l = Wo_l V_l of EVERY layer in one launch (it depends on the text memory only, not on h)
  // the fold on compensated operands as prepare() set it up - unless class CWO was switched off since: then the unfolded path
  const bool fold3 = fold3_ && x3(SAMAUDIO_CLS_CWO);
  const int fold_ltp = fold3_ && !fold3 ? 0 : fold_ltp_;
  const bool fold_all = fold_ltp && !fold3 && cfg_.n_layers <= kMaxFoldLayers && !debug_flag(DBG_FOLD_PER_LAYER);   // (one launch per layer: A/B, tests)
  if (fold3) {   // x3 context: U = Wo V of every layer on split operands, [L][rows][D][3 kp] = [U_hi | U_lo | U_hi]
    const float* wos[kMaxFoldLayers];
    for (int l = 0; l < cfg_.n_layers; ++l) wos[l] = (const float*)layers_[l].c_wo.w;
    SA_TRY(op("cross_attn_fold3", ((double)D * D * 4 + (double)rows * D * fold_kp_ * 6 + (double)Mt * D * 4) * cfg_.n_layers, 0, st, [&] {
      return launch_cross_attn_fold3_layers(wos, cfg_.n_layers, (const float*)d_.kvc, kv_ld, d_.ut3, fold_kp_, rows, Lt, fold_ltp_, H, st);
    }));
  }
  const size_t ut_layer = (size_t)rows * D * fold_kp_ * esz_;
  if (fold_all) {
    const void* wos[kMaxFoldLayers];
    for (int l = 0; l < cfg_.n_layers; ++l) wos[l] = layers_[l].c_wo.w;
    SA_TRY(op("cross_attn_fold", ((double)D * D + (double)rows * D * fold_kp_ + (double)Mt * D) * esz_ * cfg_.n_layers, 0, st, [&] {
      return launch_cross_attn_fold_layers(wos, cfg_.n_layers, d_.kvc, kv_ld, d_.ut, fold_kp_, rows, Lt, fold_ltp_, H, st);
    }));
  }
  // SAMAUDIO_OPT_PREFETCH_ROWS: a launch's idle workgroups read the next big GEMM's weights (gemm8.hip prefetch_lines).  Chain per
  // layer: qkv -> wo -> c_wq -> c_wo (read by the fold kernel); w13 -> w2 -> the next layer's qkv.  Nobody prefetches w13: the only
  // launch in front of it with idle CUs is the folded cross-attention GEMM (K = 192: 15 us), which the 85 MB read stretched to 27 us,
  // and w13 itself (236 tiles of 256 x 256) measured the same warm or cold (round 5, profiles/r5_call2/).
  const bool pf_on = bf16_ && prefetch_rows_ > 0 && M <= prefetch_rows_;
  auto prefetch = [&](GemmParams& p, const void* w_next, double elems) {
    if (pf_on && w_next) { p.pf_ptr = w_next; p.pf_bytes = (long)(elems * esz_); }
  };
  // the modulated RMSNorm in front of class `cls` of layer l (k = 0: the attention norm, QKV; k = 1: the FFN norm, W13) and the scan of
  // its output; `pre`: it writes the class's split operand [lo | hi | hi] itself
  auto norm_for = [&](int l, int k, int cls, bool pre) -> Status {
    const LayerW& w = layers_[l];
    const float* tab = w.mod_table + 3 * k * D;
    const float* gs = d_.modgs + (2L * l + k) * nt * 2 * D;
    SA_TRY(op("rmsnorm_mod", MD * (4 + (pre ? 6 : esz_)), 0, st, [&] {
      if (pre) return launch_rmsnorm_gs_split3(d_.h, gs, gs_ld, d_.x3a, (int)M, D, T, eps, st);
      if (mod_gs) return launch_rmsnorm_gs(d_.h, gs, gs_ld, d_.xn, bf16_, (int)M, D, T, eps, st, alt16(cls));
      return launch_rmsnorm_mod(d_.h, k ? w.ffn_norm : w.attn_norm, tab, tab + D, d_.t0, t6, 3 * k * D, (3 * k + 1) * D, d_.xn, bf16_,
                                (int)M, D, T, eps, st);
    }));
    return sentinel(14, d_.xn, !bf16_ ? 0 : (alt16(cls) ? 2 : 1), M, D, D, st);
  };
  // h += P . U of one layer, the batched GEMM of either fold: P [rows][T][K] probabilities, U [rows][D][K] = Wo V per batch item
  auto fold_gemm = [&](const void* P, const void* U, int K) {
    GemmParams p = lin(P, K, U, T, D, K);
    p.nbatch = rows; p.a_bstride = (long)T * K; p.w_bstride = (long)D * K;
    with_res(p, d_.h, D);
    out_f32(p, d_.h, D);
    p.res_bstride = p.f32_bstride = (long)T * D;
    return p;
  };
  for (int l = 0; l < cfg_.n_layers; ++l) {  // DiTBlock.forward, transformer.py:354-391
    const LayerW& w = layers_[l];
    const float* tab = w.mod_table;
    // self-attention branch
    // compensated operands (fp32 contexts): the producers write the split form [lo | hi | hi] themselves where they can
    const bool qkv_pre = x3(SAMAUDIO_CLS_QKV) && mod_gs, w13_pre = x3(SAMAUDIO_CLS_W13) && mod_gs;
    const bool wo_pre = x3(SAMAUDIO_CLS_WO) && x3(SAMAUDIO_X3_ATTENTION);
    bool w2_pre = false;   // (decided with the w13 launch below)
    SA_TRY(norm_for(l, 0, SAMAUDIO_CLS_QKV, qkv_pre));
    {
      GemmParams p = lin(d_.xn, D, nullptr, M, 3 * D, D);
      prefetch(p, w.wo.w, (double)D * D);
      out_act(p, d_.qkv, 3L * D);
      SA_TRY(linear(p, w.wqkv, SAMAUDIO_CLS_QKV, st, qkv_pre ? d_.x3a : nullptr));
    }
    SA_TRY(op("qkv_prep", 2 * 3 * MD * esz_, 0, st, [&] {
      if (x3(SAMAUDIO_X3_ATTENTION) && hd == 128)   // fp32 tensors, the fast access pattern (its consumer is the compensated attention)
        return launch_qkv_prep_f32x((const float*)d_.qkv, w.q_norm, w.k_norm, g_.rope_cos, g_.rope_sin, (float*)d_.Q, (float*)d_.K,
                                    (float*)d_.Vt, rows, T, Tp, H, eps, st);
      return launch_qkv_prep(d_.qkv, w.q_norm, w.k_norm, g_.rope_cos, g_.rope_sin, d_.Q, d_.K, d_.Vt, bf16_, rows, T, Tp, H,
                             eps, st, hd);
    }));
    trace("  xn", d_.xn, (size_t)M * D, bf16_, st);
    trace("  qkv", d_.qkv, (size_t)M * 3 * D, bf16_, st);
    trace("  Q", d_.Q, (size_t)rows * Tp * D, bf16_, st);
    trace("  K", d_.K, (size_t)rows * Tp * D, bf16_, st);
    trace("  Vt", d_.Vt, (size_t)rows * Tp * D, bf16_, st);
    if (x3(SAMAUDIO_X3_ATTENTION))
      SA_TRY(op("self_attention_x3", 4 * MD * 4, 4.0 * T * T * D * rows, st, [&] {
        return launch_self_attention_x3((const float*)d_.Q, (const float*)d_.K, (const float*)d_.Vt, d_.pad_mask, (float*)d_.attn, rows,
                                        T, Tp, H, hd, st, wo_pre ? d_.x3a : nullptr);
      }));
    else
    SA_TRY(op("self_attention", 4 * MD * esz_, 4.0 * T * T * D * rows, st, [&] {
      return launch_self_attention_hd(d_.Q, d_.K, d_.Vt, d_.pad_mask, d_.attn, bf16_, rows, T, Tp, H, hd, st, alt16(SAMAUDIO_CLS_WO));
    }));
    trace("  attn", d_.attn, (size_t)M * D, bf16_, st);
    SA_TRY(sentinel(15, d_.attn, !bf16_ ? 0 : (alt16(SAMAUDIO_CLS_WO) ? 2 : 1), M, D, D, st));
    {
      GemmParams p = lin(d_.attn, D, nullptr, M, D, D);  // h = x + gate_msa * attn
      p.gate_tab = tab + 2 * D; p.gate = d_.t0 + 2 * D; p.gate_ld = t6; p.rows_per_gate = T;
      with_res(p, d_.h, D);
      out_f32(p, d_.h, D);
      out_act(p, d_.hbf, D);
      if (alt16(SAMAUDIO_CLS_CWQ)) p.flags |= GEMM_FLAG_OUT_ALT;   // hbf is c_wq's operand
      prefetch(p, w.c_wq.w, (double)D * D);
      if (x3(SAMAUDIO_CLS_WO)) { p.out_act = nullptr; p.act_ld = 0; }   // (fp32 outputs only: c_wq then reads h itself)
      SA_TRY(linear(p, w.wo, SAMAUDIO_CLS_WO, st, wo_pre ? d_.x3a : nullptr));
    }
    trace("  h after wo", d_.h, (size_t)M * D, false, st);
    trace("  hbf", d_.hbf, (size_t)M * D, bf16_, st);
    // cross-attention branch: h = h + CA(h, y)   (no norm, no gate: quirk Q4)
    {
      // (an fp32 context whose wo ran on compensated operands has no second copy of h)
      GemmParams p = lin(x3(SAMAUDIO_CLS_WO) ? (const void*)d_.h : d_.hbf, D, nullptr, M, D, D);
      if (!fold_all) prefetch(p, w.c_wo.w, (double)D * D);   // (read by the per-layer fold kernel)
      out_act(p, d_.qc, D);
      SA_TRY(linear(p, w.c_wq, SAMAUDIO_CLS_CWQ, st));
    }
    const void* kv_l = (const char*)d_.kvc + (size_t)l * 2 * D * esz_;
    if (fold3) {
      // h += P . U on compensated operands: K' = 3 kp = 576 instead of 3 D
      SA_TRY(op("cross_attn_probs3", (MD * 4 + (double)M * fold_kp_ * 6 + (double)Mt * 2 * D * 4), 0, st, [&] {
        return launch_cross_attn_probs3((const float*)d_.qc, w.c_q_norm, (const float*)kv_l, kv_ld, d_.text_mask, d_.x3p, fold_kp_, rows, T, Lt,
                                        fold_ltp_, H, eps, st);
      }));
      const int K3 = 3 * fold_kp_;
      const GemmParams p = fold_gemm(d_.x3p, (const char*)d_.ut3 + (size_t)l * rows * D * K3 * 2, K3);
      SA_TRY(gemm(p, st, 2.0 * M * (double)D * H * Lt, SAMAUDIO_CLS_CWO, GemmKind::X3));
    } else if (fold_ltp) {
      // h += P . U with U = Wo V folded per (batch, head, token): K = H*Lt instead of D (see attention.hip)
      SA_TRY(op("cross_attn_probs", (MD + (double)M * fold_kp_ + (double)Mt * 2 * D) * esz_, 0, st, [&] {
        return launch_cross_attn_probs(d_.qc, w.c_q_norm, kv_l, kv_ld, d_.text_mask, d_.probs, fold_kp_, rows, T, Lt,
                                       fold_ltp_, H, eps, st);
      }));
      const void* ut_l = fold_all ? (const void*)((const char*)d_.ut + (size_t)l * ut_layer) : d_.ut;
      if (!fold_all)
        SA_TRY(op("cross_attn_fold", ((double)D * D + (double)rows * D * fold_kp_ + (double)Mt * D) * esz_, 0, st, [&] {
          return launch_cross_attn_fold(w.c_wo.w, kv_l, kv_ld, d_.ut, fold_kp_, rows, Lt, fold_ltp_, H, st);
        }));
      const GemmParams p = fold_gemm(d_.probs, ut_l, fold_kp_);
      trace("  probs", d_.probs, (size_t)M * fold_kp_, bf16_, st);
      trace("  ut", ut_l, (size_t)rows * D * fold_kp_, bf16_, st);
      SA_TRY(gemm(p, st, -1.0, SAMAUDIO_CLS_CWO));
    } else {
      SA_TRY(op("cross_attention", (2 * MD + (double)Mt * 2 * D) * esz_, 4.0 * M * Lt * D, st, [&] {
        return launch_cross_attention(d_.qc, w.c_q_norm, kv_l, kv_ld, d_.text_mask, d_.ca, bf16_, rows, T, Lt, H, eps, st, hd);
      }));
      GemmParams p = lin(d_.ca, D, nullptr, M, D, D);
      with_res(p, d_.h, D);
      out_f32(p, d_.h, D);
      SA_TRY(linear(p, w.c_wo, SAMAUDIO_CLS_CWO, st));
    }
    trace("  qc", d_.qc, (size_t)M * D, bf16_, st);
    trace("  h after cross", d_.h, (size_t)M * D, false, st);
    // feed-forward branch
    SA_TRY(norm_for(l, 1, SAMAUDIO_CLS_W13, w13_pre));
    {
      GemmParams p = lin(d_.xn, D, nullptr, M, 2 * F, D);
      p.swiglu = 1;
      out_act(p, d_.u, F);
      if (alt16(SAMAUDIO_CLS_W2)) p.flags |= GEMM_FLAG_OUT_ALT;    // u is w2's operand
      prefetch(p, w.w2.w, (double)D * F);
      // the SwiGLU epilogue writes w2's split operand itself where the 8-phase family takes the launch gemm() would make of it
      // (F % 32 == 0 among others); otherwise w2 splits u with the stand-alone kernel
      w2_pre = x3(SAMAUDIO_CLS_W13) && x3(SAMAUDIO_CLS_W2) &&
               x3_w2_pre(p, d_.x3a, w.w13, d_.x3u, d_.x3u_bytes, M, F,
                         [&](const GemmParams& q) { return launch_params(q, SAMAUDIO_CLS_W13, GemmKind::X3); });
      if (w2_pre) { p.out_act = d_.x3u; p.flags |= GEMM_FLAG_OUT_SPLIT3; }
      SA_TRY(linear(p, w.w13, SAMAUDIO_CLS_W13, st, w13_pre ? d_.x3a : nullptr));
      trace("  xn (ffn)", d_.xn, (size_t)M * D, bf16_, st);
      trace("  u", d_.u, (size_t)M * F, bf16_, st);
      p = lin(d_.u, F, nullptr, M, D, F);  // out = h + gate_mlp * ff
      p.gate_tab = tab + 5 * D; p.gate = d_.t0 + 5 * D; p.gate_ld = t6; p.rows_per_gate = T;
      with_res(p, d_.h, D);
      out_f32(p, d_.h, D);
      if (l + 1 < cfg_.n_layers) prefetch(p, layers_[l + 1].wqkv.w, 3.0 * D * D);
      SA_TRY(linear(p, w.w2, SAMAUDIO_CLS_W2, st, w2_pre ? d_.x3u : nullptr, true));
      trace("  h after ffn", d_.h, (size_t)M * D, false, st);
    }
  }
  trace("h after layers", d_.h, (size_t)M * D, false, st);
  // final modulated norm + output projection                         (transformer.py:507-519)
  {
    const bool f = f32c(SAMAUDIO_CLS_OUT);   // exact fp32: the result is the ODE's vector field itself
    void* xn = f ? (void*)d_.xn32 : d_.xn;
    SA_HIP(launch_rmsnorm_mod(d_.h, g_.final_norm, g_.final_table, g_.final_table + D, d_.t_emb, t1, 0, 0, xn,
                              f ? false : bf16_, (int)M, D, T, eps, st));
    GemmParams p = lin(xn, D, f ? (const void*)g32_.w_out : g_.w_out, M, C2, D);
    p.alpha = alpha;
    if (res) with_res(p, res, C2);
    out_f32(p, out, C2);
    SA_TRY(gemm(p, st, -1.0, SAMAUDIO_CLS_OUT, f32_if(f)));
  }
  // windowed solve: the overlapping frames of neighbouring window rows leave every evaluation with the same value (out = res + alpha *
  // field is linear in the field and res is equal in both rows, so blending `out` blends the field: DESIGN.md section 10.7).  Bytes: two
  // reads and two writes per pair if every row had a successor (the table lives on the device: an upper bound)
  if (win_next_)
    SA_TRY(op("window_blend", 16.0 * rows * win_overlap_ * C2, 3.0 * rows * win_overlap_ * C2, st,
              [&] { return launch_window_blend(out, win_next_, rows, T, win_overlap_, C2, st); }));
  hash_stage("field out", out, (size_t)M * C2 * 4, st);
  return Status{};
}

Status Engine::set_windows(const int32_t* next_row, int rows, int overlap) {
  win_next_ = nullptr;
  win_overlap_ = 0;
  win_groups_ = nullptr;   // groups are groups of window rows: they go with the table
  win_owner_ = nullptr;
  win_n_groups_ = 0;
  if (!next_row) return Status{};
  if (!prepared_) return fail(SAMAUDIO_ERR_STATE, "set_windows: call samaudio_prepare first");
  if (rows != rows_) return fail(SAMAUDIO_ERR_ARG, "set_windows: rows is not the prepared row count");
  if (overlap < 1 || overlap > frames_ / 2) return fail(SAMAUDIO_ERR_ARG, "set_windows: overlap must be in [1, frames / 2]");
  if (cfg_.latent_channels % 4) return fail(SAMAUDIO_ERR_ARG, "set_windows: latent_channels % 4 != 0");
  if (reinterpret_cast<uintptr_t>(next_row) & 3) return fail(SAMAUDIO_ERR_ARG, "set_windows: the table must be aligned to 4 bytes");
  if (!launch_window_blend) return fail(SAMAUDIO_ERR_STATE, "set_windows: this build has no window_blend_kernel");
  win_next_ = next_row;
  win_overlap_ = overlap;
  return Status{};
}

Status Engine::set_window_groups(const int32_t* groups, int n_groups, const uint8_t* owner_mask) {
  win_groups_ = nullptr;
  win_owner_ = nullptr;
  win_n_groups_ = 0;
  if (!groups) return Status{};
  if (!prepared_ || !win_next_) return fail(SAMAUDIO_ERR_STATE, "set_window_groups: call samaudio_set_windows first");
  if (n_groups < 1 || n_groups > rows_) return fail(SAMAUDIO_ERR_ARG, "set_window_groups: n_groups must be in [1, rows]");
  if (!owner_mask) return fail(SAMAUDIO_ERR_ARG, "set_window_groups: the ownership mask is missing");
  if (reinterpret_cast<uintptr_t>(groups) & 3) return fail(SAMAUDIO_ERR_ARG, "set_window_groups: the table must be aligned to 4 bytes");
  if (!launch_ode_control_groups) return fail(SAMAUDIO_ERR_STATE, "set_window_groups: this build has no ode_control_groups_kernel");
  win_groups_ = groups;
  win_owner_ = owner_mask;
  win_n_groups_ = n_groups;
  return Status{};
}

Status Engine::forward(const float* noisy, const float* time, int n_time, float* out, hipStream_t st) {
  if (!noisy || !time || !out) return fail(SAMAUDIO_ERR_ARG, "forward: null pointer");
  const Status s = eval_field(noisy, time, n_time, out, nullptr, 1.f, st);
  if (hash_on()) hash_flush((HashTrace*)hash_, this, st);
  return s;
}

// Explicit Runge-Kutta methods of torchdiffeq's fixed-grid family.  Stage i of a step t0 -> t1 = t0 + dt
// evaluates k_i = f(t0 + c_i dt, y0 + dt * sum_j a_ij k_j); then y1 = y0 + dt * bscale * sum_j b_j k_j.  Coefficients in torchdiffeq's
// grouping: rk4 is its rk4_alt_step_func (the 3/8 rule, last stage at the grid point t1), heun3 its Heun3 tableau.
struct Engine::RkTableau {
  int stages;
  float c[4];
  float a[4][4];
  float b[4], bscale;
  bool last_at_t1;
};
static const Engine::RkTableau* rk_tableau(int method) {
  static const Engine::RkTableau rk4 = {4, {0.f, 1.f / 3, 2.f / 3, 1.f}, {{}, {1.f / 3}, {-1.f / 3, 1.f}, {1.f, -1.f, 1.f}},
                                        {1.f, 3.f, 3.f, 1.f}, 0.125f, true};
  static const Engine::RkTableau heun3 = {3, {0.f, 1.f / 3, 2.f / 3}, {{}, {1.f / 3}, {0.f, 2.f / 3}}, {0.25f, 0.f, 0.75f}, 1.f,
                                          false};
  return method == SAMAUDIO_ODE_RK4 ? &rk4 : method == SAMAUDIO_ODE_HEUN3 ? &heun3 : nullptr;
}
static size_t stage_stride(int rows, int frames, int C2) { return ((size_t)rows * frames * C2 * 4 + 255) & ~size_t(255); }

// The embedded pairs of the adaptive methods: scipy.integrate's RK45 (Dormand-Prince 5(4)) and RK23
// (Bogacki-Shampine 3(2)) tableaux, rounded to fp32.  Both are FSAL: row `stages` of `a` is `b`, its evaluation at the candidate
// is K[stages], the last term of the error estimate and the next step's K[0].
struct Engine::AdaptiveTableau {
  int stages, order;               // evaluations per trial step; order of the error estimator
  float c[kOdeMaxSrc];             // c[stages] = 1
  float a[kOdeMaxSrc][kOdeMaxSrc];
  float e[kOdeMaxSrc];
};
#define Q(n, d) (float)((double)(n) / (double)(d))
static const Engine::AdaptiveTableau* adaptive_tableau(int method) {
  static const Engine::AdaptiveTableau dopri5 = {
      6, 4, {0.f, Q(1, 5), Q(3, 10), Q(4, 5), Q(8, 9), 1.f, 1.f},
      {{},
       {Q(1, 5)},
       {Q(3, 40), Q(9, 40)},
       {Q(44, 45), Q(-56, 15), Q(32, 9)},
       {Q(19372, 6561), Q(-25360, 2187), Q(64448, 6561), Q(-212, 729)},
       {Q(9017, 3168), Q(-355, 33), Q(46732, 5247), Q(49, 176), Q(-5103, 18656)},
       {Q(35, 384), 0.f, Q(500, 1113), Q(125, 192), Q(-2187, 6784), Q(11, 84)}},
      {Q(-71, 57600), 0.f, Q(71, 16695), Q(-71, 1920), Q(17253, 339200), Q(-22, 525), Q(1, 40)}};
  static const Engine::AdaptiveTableau bosh3 = {
      3, 2, {0.f, Q(1, 2), Q(3, 4), 1.f},
      {{}, {Q(1, 2)}, {0.f, Q(3, 4)}, {Q(2, 9), Q(1, 3), Q(4, 9)}},
      {Q(5, 72), Q(-1, 12), Q(-1, 9), Q(1, 8)}};
  return method == SAMAUDIO_ODE_DOPRI5 ? &dopri5 : method == SAMAUDIO_ODE_BOSH3 ? &bosh3 : nullptr;
}
#undef Q
static size_t pad256(size_t n) { return (n + 255) & ~size_t(255); }
static int ode_chunks(int frames, int C2) { return (int)(((long)frames * C2 + kOdeChunk - 1) / kOdeChunk); }

// the caller's stage buffer of an adaptive solve, carved: K[0 .. stages], the candidate, one control block per row, the time table
// [stages + 1][rows], two sets of norm partials [rows][chunks] and the word the host reads after every trial step
struct Engine::AdaptiveBufs {
  float* k[kOdeMaxSrc];
  float *ynew, *times, *part, *part_b;
  OdeRowCtl* ctl;
  int* active;
  size_t bytes;
};
Engine::AdaptiveBufs Engine::adaptive_carve(const AdaptiveTableau& tab, int rows, int frames) const {
  AdaptiveBufs b{};
  char* p = (char*)stages_;
  size_t off = 0;
  auto take = [&](size_t n) { char* q = p + off; off += pad256(n); return q; };
  const size_t state = (size_t)rows * frames * cfg_.latent_channels * 4;
  for (int i = 0; i <= tab.stages; ++i) b.k[i] = (float*)take(state);
  b.ynew = (float*)take(state);
  b.ctl = (OdeRowCtl*)take((size_t)rows * sizeof(OdeRowCtl));
  b.times = (float*)take((size_t)(tab.stages + 1) * rows * 4);
  const size_t part = (size_t)rows * ode_chunks(frames, cfg_.latent_channels) * 4;
  b.part = (float*)take(part);
  b.part_b = (float*)take(part);
  b.active = (int*)take(4);
  b.bytes = off;
  return b;
}

size_t Engine::ode_stage_bytes(int method, int rows, int frames) const {
  if (const AdaptiveTableau* ad = adaptive_tableau(method))
    return rows <= 0 || frames <= 0 ? 0 : adaptive_carve(*ad, rows, frames).bytes;
  const RkTableau* tab = rk_tableau(method);
  if (!tab || rows <= 0 || frames <= 0) return 0;
  return (size_t)tab->stages * stage_stride(rows, frames, cfg_.latent_channels);
}

Status Engine::set_ode_stages(void* p, size_t bytes) {
  if (reinterpret_cast<uintptr_t>(p) & 255) return fail(SAMAUDIO_ERR_WORKSPACE, "ode stage buffer must be 256-byte aligned");
  stages_ = (float*)p;
  stages_bytes_ = p ? bytes : 0;
  return Status{};
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return pa && pb && pa < pb + nb && pb < pa + na;
}

Status Engine::ode_solve(float* y, int method, const float* grid, int n_grid, hipStream_t st) {
  if (!prepared_) return fail(SAMAUDIO_ERR_STATE, "ode_solve: call samaudio_prepare first");
  const RkTableau* rk = rk_tableau(method);
  if (method != SAMAUDIO_ODE_EULER && method != SAMAUDIO_ODE_MIDPOINT && !rk)
    return fail(SAMAUDIO_ERR_ARG, "ode_solve: unsupported method");
  // the evaluation times go into d_.times (4096 floats): two per grid point for euler / midpoint, one per stage and step for rk4 / heun3
  const bool fits = rk ? (long)rk->stages * (n_grid - 1) <= 4096 : 2 * n_grid <= 4096;
  if (!y || !grid || n_grid < 2 || !fits) return fail(SAMAUDIO_ERR_ARG, "ode_solve: bad grid");
  for (int k = 0; k + 1 < n_grid; ++k)
    if (!(grid[k + 1] > grid[k])) return fail(SAMAUDIO_ERR_ARG, "ode_solve: grid must be increasing");
  if (!rk) return solve_launches(y, method, grid, n_grid, st);
  if (!launch_ode_stage) return fail(SAMAUDIO_ERR_STATE, "ode_solve: rk4 / heun3 are not available in this build (no ode_stage_kernel)");
  const size_t need = ode_stage_bytes(method, rows_, frames_);
  if (!stages_ || stages_bytes_ < need)
    return fail(SAMAUDIO_ERR_WORKSPACE, "ode_solve: rk4 / heun3 need samaudio_ode_stage_bytes() of stage buffers (samaudio_set_ode_stages)");
  if (overlaps(stages_, need, ws_, ws_bytes_) || overlaps(stages_, need, y, (size_t)rows_ * frames_ * cfg_.latent_channels * 4))
    return fail(SAMAUDIO_ERR_WORKSPACE, "ode_solve: the stage buffers overlap the workspace or the state");
  return solve_rk(y, *rk, grid, n_grid, st);
}

Status Engine::solve_rk(float* y, const RkTableau& tab, const float* grid, int n_grid, hipStream_t st) {
  const int s = tab.stages, steps = n_grid - 1;
  const long n = (long)rows_ * frames_ * cfg_.latent_channels;
  // stage times in torchdiffeq's float arithmetic (t0 + dt * c); all of them as kernel arguments: no host synchronisation
  std::vector<float> ev((size_t)s * steps);
  for (int k = 0; k < steps; ++k) {
    const float t0 = grid[k], dt = grid[k + 1] - grid[k];
    for (int i = 0; i < s; ++i)
      ev[(size_t)s * k + i] = i == 0 ? t0 : (i == s - 1 && tab.last_at_t1) ? grid[k + 1] : t0 + dt * tab.c[i];
  }
  SA_HIP(launch_set_floats(d_.times, ev.data(), (int)ev.size(), st));
  float* kbuf[4];
  for (int i = 0; i < s; ++i) kbuf[i] = (float*)((char*)stages_ + i * stage_stride(rows_, frames_, cfg_.latent_channels));
  for (int k = 0; k < steps; ++k) {
    const float dt = grid[k + 1] - grid[k];
    for (int i = 0; i < s; ++i) {
      // k_i = f(t_i, stage input): stage 0 reads y0 itself, the others the combination the previous stage left in d_.ymid
      SA_TRY(eval_field(i == 0 ? y : d_.ymid, d_.times + (size_t)s * k + i, 1, kbuf[i], nullptr, 1.f, st));
      // then the next stage's input, or after the last stage y1 written over y0
      const bool last = i == s - 1;
      OdeStageArgs a{};
      for (int j = 0; j <= i; ++j) {
        const float c = last ? tab.b[j] : tab.a[i + 1][j];
        if (c != 0.f) {
          a.k[a.n_src] = kbuf[j];
          a.coef[a.n_src++] = c;
        }
      }
      const float scale = last ? dt * tab.bscale : dt;
      float* out = last ? y : d_.ymid;
      SA_TRY(op("ode_stage", (a.n_src + 2.0) * n * 4, 2.0 * (a.n_src + 1) * n, st,
                [&] { return launch_ode_stage(y, a, scale, out, n, st); }));
    }
  }
  if (hash_on()) hash_flush((HashTrace*)hash_, this, st);
  return Status{};
}

bool ode_control_args(int method, float t0, float t1, const samaudio_ode_adaptive& opt, OdeControlArgs& ca) {
  const Engine::AdaptiveTableau* tab = adaptive_tableau(method);
  if (!tab) return false;
  ca = OdeControlArgs{};
  ca.t0 = t0; ca.t1 = t1; ca.first_step = opt.first_step;
  ca.safety = opt.safety; ca.ifactor = opt.ifactor; ca.dfactor = opt.dfactor;
  ca.order = tab->order; ca.max_num_steps = opt.max_num_steps; ca.n_times = tab->stages + 1;
  for (int i = 0; i <= tab->stages; ++i) ca.c[i] = tab->c[i];
  return true;
}

// Adaptive solve: every row integrates from t0 to t1 with its own time, step and accept / reject decision, all
// of them on the device.  One trial step = the stage evaluations of all rows (per-row times: eval_field with n_time = rows), the error
// norms, the controller, the commit, then ONE host read: the number of rows still running.  Rows that have ended ride along - the stage
// kernel hands their state through, the field evaluates it at their own time, and nothing of theirs is written - until the last row ends.
// With windows and a group table set the unit of step control is the group instead of the row (section 10.11).
Status Engine::ode_solve_adaptive(float* y, int method, float t0, float t1, const samaudio_ode_adaptive* opt,
                                  samaudio_ode_row_stats* stats, hipStream_t st) {
  if (!prepared_) return fail(SAMAUDIO_ERR_STATE, "ode_solve_adaptive: call samaudio_prepare first");
  const AdaptiveTableau* tab = adaptive_tableau(method);
  if (!tab) return fail(SAMAUDIO_ERR_ARG, "ode_solve_adaptive: the method must be SAMAUDIO_ODE_DOPRI5 or SAMAUDIO_ODE_BOSH3");
  if (!y || !opt || !stats) return fail(SAMAUDIO_ERR_ARG, "ode_solve_adaptive: null pointer");
  if (!(t1 > t0)) return fail(SAMAUDIO_ERR_ARG, "ode_solve_adaptive: t1 must lie behind t0");
  if (!(opt->rtol > 0.f) || !(opt->atol > 0.f)) return fail(SAMAUDIO_ERR_ARG, "ode_solve_adaptive: rtol and atol must be positive");
  if (!(opt->safety > 0.f) || !(opt->ifactor >= 1.f) || !(opt->dfactor > 0.f) || !(opt->dfactor < 1.f) || opt->max_num_steps < 1 ||
      opt->first_step != opt->first_step)
    return fail(SAMAUDIO_ERR_ARG, "ode_solve_adaptive: safety > 0, ifactor >= 1, 0 < dfactor < 1, max_num_steps >= 1");
  if (cfg_.latent_channels % 4) return fail(SAMAUDIO_ERR_ARG, "ode_solve_adaptive: latent_channels % 4 != 0");
  if (win_next_ && !win_groups_)
    return fail(SAMAUDIO_ERR_STATE, "ode_solve_adaptive: windows are set (rows of one clip must share their times: "
                                    "samaudio_set_window_groups gives them step control per clip)");
  if (!launch_ode_stage_rows || !launch_ode_error || !launch_ode_control || !launch_ode_commit)
    return fail(SAMAUDIO_ERR_STATE, "ode_solve_adaptive: dopri5 / bosh3 are not available in this build (no ode_*_rows kernels)");
  const int rows = rows_, T = frames_, C2 = cfg_.latent_channels, S = tab->stages;
  const size_t need = ode_stage_bytes(method, rows, T);
  if (!stages_ || stages_bytes_ < need)
    return fail(SAMAUDIO_ERR_WORKSPACE,
                "ode_solve_adaptive: dopri5 / bosh3 need samaudio_ode_stage_bytes() of stage buffers (samaudio_set_ode_stages)");
  if (overlaps(stages_, need, ws_, ws_bytes_) || overlaps(stages_, need, y, (size_t)rows * T * C2 * 4))
    return fail(SAMAUDIO_ERR_WORKSPACE, "ode_solve_adaptive: the stage buffers overlap the workspace or the state");
  const AdaptiveBufs b = adaptive_carve(*tab, rows, T);
  phase_ = Phase::Dit;   // (the profile label of the launches ahead of the first evaluation)
  const long row_elems = (long)T * C2;
  const double n = (double)rows * row_elems;
  const int chunks = ode_chunks(T, C2);
  OdeControlArgs ca{};
  ode_control_args(method, t0, t1, *opt, ca);
  // windows with a group table: the same launches, with the norm over the frames a row OWNS and one
  // controller lane per (clip, candidate) that hands all its window rows the same time, step and decision
  const bool grouped = win_next_ && win_groups_;
  const uint8_t* const norm_mask = grouped ? win_owner_ : d_.pad_mask;

  auto control = [&](int mode) {
    if (grouped)
      return op("ode_control_groups", (2.0 * sizeof(OdeRowCtl) + 4.0 * chunks) * rows, 0, st, [&] {
        return launch_ode_control_groups(b.ctl, mode, ca, b.part, b.part_b, chunks, norm_mask, T, C2, b.times, b.active, rows,
                                         win_groups_, win_n_groups_, st);
      });
    return op("ode_control", (2.0 * sizeof(OdeRowCtl) + 4.0 * chunks) * rows, 0, st, [&] {
      return launch_ode_control(b.ctl, mode, ca, b.part, b.part_b, chunks, d_.pad_mask, T, C2, b.times, b.active, rows, st);
    });
  };
  // sources = the K rows with a non-zero weight among w[0 .. count)
  auto sources = [&](const float* w, int count) {
    OdeSrcArgs a{};
    for (int j = 0; j < count; ++j)
      if (w[j] != 0.f) {
        a.k[a.n_src] = b.k[j];
        a.coef[a.n_src++] = w[j];
      }
    return a;
  };
  auto combine = [&](const OdeSrcArgs& a, float* out) {
    return op("ode_stage_rows", (a.n_src + 2.0) * n * 4, 2.0 * (a.n_src + 1) * n, st,
              [&] { return launch_ode_stage_rows(y, a, b.ctl, out, rows, row_elems, st); });
  };
  auto norm = [&](const OdeSrcArgs& a, const float* ynew, int use_h, float* part) {
    return op("ode_error", (a.n_src + (ynew ? 2.0 : 1.0)) * n * 4, 2.0 * (a.n_src + 4) * n, st, [&] {
      return launch_ode_error(y, ynew, a, b.ctl, norm_mask, opt->rtol, opt->atol, use_h, part, rows, T, C2, st);
    });
  };
  auto field = [&](const float* in, int slot, float* out) {
    return eval_field(in, b.times + (size_t)slot * rows, rows, out, nullptr, 1.f, st);
  };
  int evaluations = 0, active = rows;
  auto read_active = [&]() -> Status {
    SA_HIP(hipMemcpyAsync(&active, b.active, sizeof(int), hipMemcpyDeviceToHost, st));
    SA_HIP(hipStreamSynchronize(st));
    return Status{};
  };

  SA_TRY(control(ODE_CTL_RESET));
  SA_TRY(field(y, 0, b.k[0]));   // K[0] = f(t0, y0)
  ++evaluations;
  if (!(opt->first_step > 0.f)) {   // scipy's select_initial_step, with the row's own norms
    const float one[2] = {1.f, -1.f};
    OdeSrcArgs self{};
    self.k[0] = y; self.coef[0] = 1.f; self.n_src = 1;
    SA_TRY(norm(self, nullptr, 0, b.part));                  // d0 = |y0 / scale|
    SA_TRY(norm(sources(one, 1), nullptr, 0, b.part_b));     // d1 = |f0 / scale|
    SA_TRY(control(ODE_CTL_INIT1));                          // h0
    SA_TRY(combine(sources(one, 1), d_.ymid));               // y1 = y0 + h0 f0
    SA_TRY(field(d_.ymid, 1, b.k[1]));                       // f1 = f(t0 + h0, y1)
    ++evaluations;
    OdeSrcArgs diff{};
    diff.k[0] = b.k[1]; diff.k[1] = b.k[0]; diff.coef[0] = 1.f; diff.coef[1] = -1.f; diff.n_src = 2;
    SA_TRY(norm(diff, nullptr, 0, b.part));                  // d2 h0 = |(f1 - f0) / scale|
    SA_TRY(control(ODE_CTL_INIT2));
  }
  SA_TRY(read_active());
  while (active > 0) {
    for (int i = 1; i < S; ++i) {
      SA_TRY(combine(sources(tab->a[i], i), d_.ymid));
      SA_TRY(field(d_.ymid, i, b.k[i]));
    }
    SA_TRY(combine(sources(tab->a[S], S), b.ynew));          // the candidate: row S of `a` is b
    SA_TRY(field(b.ynew, S, b.k[S]));
    evaluations += S;
    SA_TRY(norm(sources(tab->e, S + 1), b.ynew, 1, b.part));
    SA_TRY(control(ODE_CTL_STEP));
    SA_TRY(op("ode_commit", 4.0 * n * 4, 0, st, [&] { return launch_ode_commit(y, b.ynew, b.k[0], b.k[S], b.ctl, rows, row_elems, st); }));
    SA_TRY(read_active());
  }
  std::vector<OdeRowCtl> host(rows);
  SA_HIP(hipMemcpyAsync(host.data(), b.ctl, (size_t)rows * sizeof(OdeRowCtl), hipMemcpyDeviceToHost, st));
  SA_HIP(hipStreamSynchronize(st));
  for (int r = 0; r < rows; ++r) {
    stats[r].accepted = host[r].accepted;
    stats[r].rejected = host[r].rejected;
    stats[r].status = host[r].status;
    stats[r].evaluations = evaluations;
    stats[r].t = host[r].t;
    stats[r].last_h = host[r].h_prev;
  }
  if (hash_on()) hash_flush((HashTrace*)hash_, this, st);
  return Status{};
}

Status Engine::solve_launches(float* y, int method, const float* grid, int n_grid, hipStream_t st) {
  std::vector<float> ev(2 * (size_t)n_grid);
  for (int k = 0; k + 1 < n_grid; ++k) {
    ev[2 * k] = grid[k];
    ev[2 * k + 1] = (float)((double)grid[k] + 0.5 * ((double)grid[k + 1] - (double)grid[k]));
  }
  SA_HIP(launch_set_floats(d_.times, ev.data(), (int)ev.size(), st));   // as kernel arguments: no host synchronisation
  for (int k = 0; k + 1 < n_grid; ++k) {
    const float dt = (float)((double)grid[k + 1] - (double)grid[k]);
    if (method == SAMAUDIO_ODE_EULER) {
      SA_TRY(eval_field(y, d_.times + 2 * k, 1, y, y, dt, st));
    } else {
      SA_TRY(eval_field(y, d_.times + 2 * k, 1, d_.ymid, y, 0.5f * dt, st));
      SA_TRY(eval_field(d_.ymid, d_.times + 2 * k + 1, 1, y, y, dt, st));
    }
  }
  if (hash_on()) hash_flush((HashTrace*)hash_, this, st);
  return Status{};
}

// ---------------------------------------------------------------------------------------------------
// DAC-VAE: every Conv1d / ConvTranspose1d is one launch of the generalised GEMM over channels-last,
// halo-padded activations; Snake is fused into the producer's epilogue (raw f32 stream for residuals,
// activated copy as the next convolution's operand).
// ---------------------------------------------------------------------------------------------------
static GemmParams conv_same(const void* x, long T, int Cin, int taps, int dil, const void* W, int Kp, int Cout,
                            int items) {
  GemmParams p = lin(x, Cin, W, T, Cout, Kp);
  p.kc = Cin;
  p.tap_stride = taps == 1 ? (long)Cin : (long)dil * Cin;
  p.a_off = (long)(HALO - (taps / 2) * dil) * Cin;
  p.a_bstride = (T + 2L * HALO) * Cin;
  p.nbatch = items;
  return p;
}
static void halo_out(GemmParams& p, float* raw, void* act, long T, int C, int actfn, const float* alpha) {
  if (raw) { p.out_f32 = raw; p.f32_bstride = (T + 2L * HALO) * C; p.f32_ld = C; p.f32_off = (long)HALO * C; }
  if (act) { p.out_act = act; p.act_bstride = (T + 2L * HALO) * C; p.act_ld = C; p.act_off = (long)HALO * C; }
  p.act = actfn;
  p.act_alpha = alpha;
}

// the buffers of one pass over n waveforms, carved from the workspace (plan_codec)
Status Engine::codec_carve(bool decode, int n, int64_t S, CodecBufs& cb) {
  Bump b(ws_, ws_bytes_);
  plan_codec(b, decode, n, S, &cb);
  if (!b.fits()) return fail(SAMAUDIO_ERR_WORKSPACE, "codec: workspace too small");
  x3_codec_scratch_ = cb.x3;
  x3_codec_scratch_bytes_ = cb.x3_bytes;
  return Status{};
}

Status Engine::res_units(const StageW& sw, SBuf& sb, int n, const float* next_alpha, hipStream_t st) {
  const long T = sb.T;
  const int C = sb.C, dil[3] = {1, 3, 9};
  for (int j = 0; j < 3; ++j) {
    const ResUnitW& r = sw.r[j];
    GemmParams p = conv_same(sb.act, T, C, 7, dil[j], r.w1, r.k1pad, C, n);
    p.bias = r.b1;
    halo_out(p, nullptr, sb.tmp, T, C, ACT_SNAKE, r.a2);
    GemmParams q = conv_same(sb.tmp, T, C, 1, 1, r.w2, r.k2pad, C, n);
    q.bias = r.b2;
    q.res = sb.raw; q.res_bstride = (T + 2L * HALO) * C; q.res_ld = C; q.res_off = (long)HALO * C;
    halo_out(q, sb.raw, sb.act, T, C, ACT_SNAKE, j < 2 ? sw.r[j + 1].a1 : next_alpha);
    SA_TRY(res_unit(p, q, sb.act, sb.tmp, 2.0 * T * C * 7 * C * n, 2.0 * T * C * C * n, st));
  }
  return Status{};
}

// ---------------------------------------------------------------------------------------------------
// Time tiles.  The codec is a stack of convolutions, so latent frame f of either direction depends on a
// bounded range of input frames: a pass over the segment [a - h, b + h) of a clip computes frames [a, b) as the whole pass does.
// ---------------------------------------------------------------------------------------------------
static long floor_div(long a, long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static long ceil_div(long a, long b) { return -floor_div(-a, b); }

// The reach of one direction in whole latent frames, walked backwards over the layers codec_encode / codec_decode launch.  While
// walking, rows [f * per - lo, f * per + hi] of the current layer's input - `per` rows to the frame - feed the outputs of frame f.
int Engine::codec_halo_frames(bool decode) const {
  long lo = 0, hi = 0, per = 1, need = 0;
  auto see = [&] { need = std::max(need, std::max(ceil_div(lo, per), ceil_div(hi - (per - 1), per))); };
  auto same = [&](int taps, int dil) { lo += (long)(taps / 2) * dil; hi += (long)(taps / 2) * dil; };
  auto units = [&] {   // the three residual units of a stage, last first: k1 behind the dilated k7
    for (int dil : {9, 3, 1}) { same(1, 1); same(7, dil); }
  };
  if (!decode) {
    same(1, 1);   // quantizer.in_proj
    same(3, 1);
    see();
    for (int i = 3; i >= 0; --i) {
      // strided convolution k = 2s, pad (s + 1) / 2: output row q reads input rows [q s - pad, q s - pad + 2s)
      const long s = cfg_.enc_rates[i], pad = (s + 1) / 2;
      lo = lo * s + pad; hi = hi * s + 2 * s - 1 - pad; per *= s;
      units();
      see();
    }
    same(7, 1);
    see();
  } else {
    per = codec_hop(cfg_);
    hi = per - 1;   // the frame's own samples
    same(7, 1);     // k7 + tanh
    see();
    for (int i = 3; i >= 0; --i) {
      units();
      see();
      // transposed convolution as codec_decode indexes it: output row o = q s + r - pad (0 <= r < s) reads input rows q - 1 and q
      const long s = cfg_.dec_rates[i], pad = (s + 1) / 2;
      lo = 1 - floor_div(pad - lo, s); hi = floor_div(hi + pad, s); per /= s;
      see();
    }
    same(7, 1);
    same(1, 1);   // quantizer.out_proj
    see();
  }
  return (int)need;
}

// tile k of a clip of T frames in tiles of L: it keeps [kL, min(T, (k + 1) L)) of a pass over [max(0, kL - h), min(T, (k + 1) L + h))
Engine::CodecSeg Engine::codec_tile(long T, long L, long h, long k) {
  CodecSeg g;
  g.keep0 = k * L; g.keep1 = std::min(T, (k + 1) * L);
  g.t0 = std::max(0L, g.keep0 - h); g.t1 = std::min(T, g.keep1 + h);
  g.T = T;
  return g;
}

int64_t Engine::codec_tile_samples(int frames, int tile_frames, bool decode) const {
  if (frames < 1 || tile_frames < 1) return -1;
  const long T = frames, L = tile_frames, h = codec_halo_frames(decode);
  long longest = 0;
  for (long k = 0; k * L < T; ++k) {
    const CodecSeg g = codec_tile(T, L, h, k);
    longest = std::max(longest, g.t1 - g.t0);
  }
  return longest * codec_hop(cfg_);
}

Status Engine::codec_encode(const float* wav, int items, int64_t S, float* latent, hipStream_t st) {
  if (!enc_ready_) return fail(SAMAUDIO_ERR_STATE, "codec_encode: codec weights not finalized");
  const long hop = codec_hop(cfg_);
  if (!wav || !latent || items <= 0 || S <= 0 || S % hop) return fail(SAMAUDIO_ERR_ARG, "codec_encode: samples % hop != 0");
  const int chunk = codec_chunk(items, S, false);
  if (chunk < 1) return fail(SAMAUDIO_ERR_WORKSPACE, "codec_encode: workspace too small");
  prepared_ = false;  // the codec scratch aliases the DiT scratch
  phase_ = Phase::Codec;
  const long T = S / hop;
  const CodecSeg whole{0, T, 0, T, T};
  for (int i0 = 0; i0 < items; i0 += chunk)
    SA_TRY(encode_pass(wav, i0, items - i0 < chunk ? items - i0 : chunk, whole, latent, st));
  return Status{};
}

Status Engine::codec_encode_tiled(const float* wav, int items, int64_t S, int tile_frames, float* latent, hipStream_t st) {
  if (tile_frames < 1) return fail(SAMAUDIO_ERR_ARG, "codec_encode_tiled: tile_frames < 1");
  const long hop = codec_hop(cfg_);
  if (S <= 0 || S % hop || tile_frames >= S / hop) return codec_encode(wav, items, S, latent, st);   // one tile: the whole pass
  if (!enc_ready_) return fail(SAMAUDIO_ERR_STATE, "codec_encode: codec weights not finalized");
  if (!wav || !latent || items <= 0) return fail(SAMAUDIO_ERR_ARG, "codec_encode_tiled: bad argument");
  const long T = S / hop, L = tile_frames, h = codec_halo_frames(false);
  const int chunk = codec_chunk(items, codec_tile_samples((int)T, tile_frames, false), false);
  if (chunk < 1) return fail(SAMAUDIO_ERR_WORKSPACE, "codec_encode_tiled: workspace too small for one segment");
  prepared_ = false;
  phase_ = Phase::Codec;
  for (int i0 = 0; i0 < items; i0 += chunk)
    for (long k = 0; k * L < T; ++k)
      SA_TRY(encode_pass(wav, i0, items - i0 < chunk ? items - i0 : chunk, codec_tile(T, L, h, k), latent, st));
  return Status{};
}

// One pass over frames [g.t0, g.t1) of the n waveforms from item i0 on; `wav` / `latent`: the whole tensors, clips of g.T frames.  Only the last
// launch knows about the kept rows [g.keep0, g.keep1): it computes those and writes them to their place in `latent`.
Status Engine::encode_pass(const float* wav, int i0, int n, const CodecSeg& g, float* latent, hipStream_t st) {
  const long hop = codec_hop(cfg_), S = (g.t1 - g.t0) * hop;
  const int CL = cfg_.codec_latent, CD = cfg_.codec_dim;
  {
    CodecBufs cb;
    SA_TRY(codec_carve(false, n, S, cb));
    SBuf* const sb = cb.sb;
    // waveform -> [n][HALO + S + HALO][8] (channel 0), zero halos
    SA_HIP(hipMemsetAsync(cb.in8, 0, (size_t)n * (S + 2 * HALO) * 8 * esz_, st));
    SA_HIP(launch_to_act(wav + ((long)i0 * g.T + g.t0) * hop, g.T * hop, 1, 0, cb.in8, 0, bf16_, n, S, 1, 8, HALO, st));
    for (int i = 0; i < 5; ++i) {
      SA_HIP(launch_zero_halo(sb[i].act, bf16_, n, sb[i].T, sb[i].C, HALO, st));
      SA_HIP(launch_zero_halo(sb[i].tmp, bf16_, n, sb[i].T, sb[i].C, HALO, st));
    }
    SA_HIP(launch_zero_halo(cb.eout, bf16_, n, sb[4].T, CL, HALO, st));
    {  // conv k7 (1 -> 64): window of 8 samples x 8 padded channels = one 64-wide row
      GemmParams p = lin(cb.in8, 8, enc_.in_w, S, sb[0].C, 64);
      p.a_off = (long)(HALO - 3) * 8; p.a_bstride = (S + 2L * HALO) * 8; p.nbatch = n; p.bias = enc_.in_b;
      halo_out(p, sb[0].raw, sb[0].act, S, sb[0].C, ACT_SNAKE, enc_.s[0].r[0].a1);
      SA_TRY(codec_gemm(p, st, 2.0 * S * sb[0].C * 7 * n));
    }
    for (int i = 0; i < 4; ++i) {
      const StageW& sw = enc_.s[i];
      const long T = sb[i].T;
      const int C = sb[i].C, s = cfg_.enc_rates[i];
      SA_TRY(res_units(sw, sb[i], n, sw.a, st));
      // strided conv k = 2s, stride s, pad s/2: the 2s input rows of one output are contiguous
      const int pad = (s + 1) / 2;
      GemmParams p = lin(sb[i].act, (long)s * C, sw.w, T / s, 2 * C, 2 * s * C);
      p.a_off = (long)(HALO - pad) * C; p.a_bstride = (T + 2L * HALO) * C; p.nbatch = n; p.bias = sw.b;
      halo_out(p, sb[i + 1].raw, sb[i + 1].act, T / s, 2 * C, ACT_SNAKE, i < 3 ? enc_.s[i + 1].r[0].a1 : enc_.out_a);
      SA_TRY(codec_gemm(p, st));
    }
    {
      const long T = sb[4].T;
      const int C = sb[4].C;
      GemmParams p = conv_same(sb[4].act, T, C, 3, 1, enc_.out_w, 3 * C, CL, n);
      p.bias = enc_.out_b;
      halo_out(p, nullptr, cb.eout, T, CL, ACT_NONE, nullptr);
      SA_TRY(codec_gemm(p, st));
      p = conv_same(cb.eout, T, CL, 1, 1, enc_.proj_w, CL, CD, n);  // quantizer.in_proj, mean half only
      p.bias = enc_.proj_b;
      p.a_off += (g.keep0 - g.t0) * CL; p.M = (int)(g.keep1 - g.keep0);   // (the whole pass: every row)
      p.out_f32 = latent + ((long)i0 * g.T + g.keep0) * CD; p.f32_bstride = g.T * CD; p.f32_ld = CD; p.f32_off = 0;
      SA_TRY(codec_gemm(p, st));
    }
  }
  return Status{};
}

Status Engine::codec_decode(const float* latent, int items, int T0, float* wav, hipStream_t st, bool pairs) {
  if (!codec_ready_) return fail(SAMAUDIO_ERR_STATE, "codec_decode: codec weights not finalized");
  if (!latent || !wav || items <= 0 || T0 <= 0) return fail(SAMAUDIO_ERR_ARG, "codec_decode: bad argument");
  if (pairs && items % 2) return fail(SAMAUDIO_ERR_ARG, "codec_decode: the state layout holds (target, residual) pairs");
  const int64_t S = (int64_t)T0 * codec_hop(cfg_);
  const int chunk = codec_chunk(items, S, pairs);
  if (chunk < 1)
    return fail(SAMAUDIO_ERR_WORKSPACE, pairs ? "codec_decode: workspace too small for one (target, residual) pair" : "codec_decode: workspace too small");
  prepared_ = false;
  phase_ = Phase::Codec;
  const CodecSeg whole{0, T0, 0, T0, T0};
  for (int i0 = 0; i0 < items; i0 += chunk)
    SA_TRY(decode_pass(latent, i0, items - i0 < chunk ? items - i0 : chunk, whole, wav, st, pairs));
  return Status{};
}

Status Engine::codec_decode_tiled(const float* latent, int items, int T0, int tile_frames, float* wav, hipStream_t st, bool pairs) {
  if (tile_frames < 1) return fail(SAMAUDIO_ERR_ARG, "codec_decode_tiled: tile_frames < 1");
  if (T0 <= 0 || tile_frames >= T0) return codec_decode(latent, items, T0, wav, st, pairs);   // one tile: the whole pass
  if (!codec_ready_) return fail(SAMAUDIO_ERR_STATE, "codec_decode: codec weights not finalized");
  if (!latent || !wav || items <= 0) return fail(SAMAUDIO_ERR_ARG, "codec_decode_tiled: bad argument");
  if (pairs && items % 2) return fail(SAMAUDIO_ERR_ARG, "codec_decode: the state layout holds (target, residual) pairs");
  const long T = T0, L = tile_frames, h = codec_halo_frames(true);
  const int chunk = codec_chunk(items, codec_tile_samples(T0, tile_frames, true), pairs);
  if (chunk < 1)
    return fail(SAMAUDIO_ERR_WORKSPACE, pairs ? "codec_decode_tiled: workspace too small for one segment of one (target, residual) pair"
                                              : "codec_decode_tiled: workspace too small for one segment");
  prepared_ = false;
  phase_ = Phase::Codec;
  for (int i0 = 0; i0 < items; i0 += chunk)
    for (long k = 0; k * L < T; ++k)
      SA_TRY(decode_pass(latent, i0, items - i0 < chunk ? items - i0 : chunk, codec_tile(T, L, h, k), wav, st, pairs));
  return Status{};
}

// One pass over frames [g.t0, g.t1) of the n waveforms from item i0 on; `latent` / `wav`: the whole tensors, clips of g.T frames.
// Only the last launch knows about the kept rows [g.keep0, g.keep1): it computes their samples and writes them to their place in `wav`.
Status Engine::decode_pass(const float* latent, int i0, int n, const CodecSeg& g, float* wav, hipStream_t st, bool pairs) {
  const long hop = codec_hop(cfg_), T0 = g.t1 - g.t0;
  const int64_t S = (int64_t)T0 * hop;
  const int CL = cfg_.codec_latent, CD = cfg_.codec_dim;
  {
    CodecBufs cb;
    SA_TRY(codec_carve(true, n, S, cb));
    SBuf* const sb = cb.sb;
    void *const lat = cb.lat, *const p0 = cb.p0;
    SA_HIP(launch_zero_halo(lat, bf16_, n, T0, CD, HALO, st));
    SA_HIP(launch_zero_halo(p0, bf16_, n, T0, CL, HALO, st));
    for (int i = 0; i < 5; ++i) {
      SA_HIP(launch_zero_halo(sb[i].act, bf16_, n, sb[i].T, sb[i].C, HALO, st));
      SA_HIP(launch_zero_halo(sb[i].tmp, bf16_, n, sb[i].T, sb[i].C, HALO, st));
    }
    if (pairs) {   // items (2b, 2b + 1) = channels [0, CD) / [CD, 2 CD) of state row block b: two strided gathers, no transposed copy
      const long item = (long)(T0 + 2 * HALO) * CD;
      for (int sgn = 0; sgn < 2; ++sgn)
        SA_HIP(launch_to_act(latent + ((long)(i0 / 2) * g.T + g.t0) * 2 * CD, g.T * 2 * CD, 2L * CD, sgn * CD, (char*)lat + (size_t)sgn * item * esz_,
                             2 * item, bf16_, n / 2, T0, CD, CD, HALO, st));
    } else
    SA_HIP(launch_to_act(latent + ((long)i0 * g.T + g.t0) * CD, g.T * CD, CD, 0, lat, 0, bf16_, n, T0, CD, CD, HALO, st));
    {
      GemmParams p = conv_same(lat, T0, CD, 1, 1, dec_.proj_w, CD, CL, n);  // quantizer.out_proj
      p.bias = dec_.proj_b;
      halo_out(p, nullptr, p0, T0, CL, ACT_NONE, nullptr);
      SA_TRY(codec_gemm(p, st));
      p = conv_same(p0, T0, CL, 7, 1, dec_.in_w, 7 * CL, sb[0].C, n);
      p.bias = dec_.in_b;
      halo_out(p, nullptr, sb[0].act, T0, sb[0].C, ACT_SNAKE, dec_.s[0].a);
      SA_TRY(codec_gemm(p, st));
    }
    for (int i = 0; i < 4; ++i) {
      const StageW& sw = dec_.s[i];
      const long Tin = sb[i].T, Tout = sb[i + 1].T;
      const int Cin = sb[i].C, C = sb[i + 1].C, s = cfg_.dec_rates[i];
      const int pad = (s + 1) / 2;
      {  // ConvTranspose1d(k=2s, stride s, pad s/2): out rows q*s + r - pad = x[q-1] W[r+s] + x[q] W[r]
        GemmParams p = lin(sb[i].act, Cin, sw.w, Tin + 1, s * C, 2 * Cin);
        p.a_off = (long)(HALO - 1) * Cin; p.a_bstride = (Tin + 2L * HALO) * Cin; p.nbatch = n;
        p.bias = sw.b; p.chan_mod = C;
        halo_out(p, sb[i + 1].raw, sb[i + 1].act, Tout, C, ACT_SNAKE, sw.r[0].a1);
        p.f32_ld = p.act_ld = (long)s * C;
        p.f32_off = p.act_off = (long)(HALO - pad) * C;
        p.c_ld_rel = (long)s * C; p.c_lo = (long)pad * C; p.c_hi = (Tout + pad) * (long)C;
        SA_TRY(codec_gemm(p, st, 2.0 * Tout * C * 2 * Cin * n));
      }
      SA_TRY(res_units(sw, sb[i + 1], n, i < 3 ? dec_.s[i + 1].a : dec_.out_a, st));
    }
    {  // conv k7 (C -> 1) + tanh
      const long T = sb[4].T;
      const int C = sb[4].C;
      GemmParams p = conv_same(sb[4].act, T, C, 7, 1, dec_.out_w, dec_.out_kpad, 1, n);
      p.bias = dec_.out_b;
      p.act = ACT_TANH; p.f32_act = 1;
      const long M = (g.keep1 - g.keep0) * hop;   // (the whole pass: every row)
      p.a_off += (g.keep0 - g.t0) * hop * C; p.M = (int)M;
      p.out_f32 = wav + ((long)i0 * g.T + g.keep0) * hop; p.f32_bstride = g.T * hop; p.f32_ld = 1; p.f32_off = 0;
      SA_TRY(codec_gemm(p, st, 2.0 * M * 7 * C * n));
    }
  }
  return Status{};
}

}  // namespace sa
