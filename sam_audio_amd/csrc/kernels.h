// Launchers of the non-GEMM kernels (kernels.hip, attention.hip).  `bf16` selects the activation
// element type AT: bf16_t (bf16 compute mode) or float (fp32 parity mode).
#pragma once
#include "common.h"

namespace sa {

// test aid: fill the LDS of every CU with NaN bit patterns (LDS persists between kernels)
hipError_t launch_poison_lds(hipStream_t st);

// test / tuning switches (samaudio_debug_set_flag, SAMAUDIO_DEBUG_FLAGS=N=V); 0 = shipped path.  The numbers are a debugging ABI (the
// tests, the tools and the logs under profiles/ use them; sam_audio_amd/hip.py mirrors the names, tests/test_gemm_names_cpu.py pins
// both).  Round 3 removed the A/B generations that had lost their measurements (the logs are under profiles/, the code in the git
// history); what is left are hooks the tests use and one-line policy thresholds.
enum DebugFlag : int {
  // 1 = k7 convolutions as implicit GEMMs, no conv7h kernel (the bitwise-equality tests of conv7h: test_gemm2_gpu.py)
  DBG_NO_CONV7H = 11,
  // 1 = DAC residual units as two launches (k7 + k1) instead of the fused resunit kernel (test_path_gpu.py)
  DBG_RESUNIT_TWO_LAUNCHES = 16,
  // 1 = fuse residual units whatever the launch size; small launches otherwise stay two launches (test_path_gpu.py)
  DBG_RESUNIT_FUSE_ALWAYS = 18,
  // residual units on the weight-stationary kernel: DBG_WS_* below (test_gemm2_gpu.py, test_path_gpu.py, tools/op_bench.py)
  DBG_RESUNIT_WS = 19,
  // 1 = gemm8s always in its plain double-buffered form; launches of <= 256 workgroups otherwise use the pipelined form (test_gemm2_gpu.py)
  DBG_GEMM8S_PLAIN = 21,
  // epilogue of the 8-phase family: DBG_EPI_* below (the bitwise-equality tests of the lean forms: test_gemm2_gpu.py)
  DBG_GEMM8_EPILOGUE = 24,
  // 1 = the 8-phase kernel launches one workgroup per tile; shipped: persistent above 256 tiles (its bitwise test: test_gemm2_gpu.py)
  DBG_GEMM8_NOT_PERSISTENT = 26,
  // wave roles of gemm8s' pipelined form (gemm8.hip): DBG_ROLES_* below (test_gemm2_gpu.py, test_fp16_gpu.py)
  DBG_GEMM8S_ROLES = 27,
  // 1 = qkv_prep with its 16-bit rounding written out: the form before round 4, reproducer of the run-to-run difference its SDWA
  // instruction sequence showed beside another kernel's waves (kernels.hip; test_isa_cpu.py needs the form, tools/stress_qkv_prep.py)
  DBG_QKV_PREP_SWROUND = 29,
  // (A/B, no test) number of 256x256 tiles from which the policy uses gemm8 instead of gemm8s (0 = shipped: 128)
  DBG_GEMM8_MIN_TILES = 30,
  // 1 = the folded cross-attention operand U = Wo V of every layer in its own launch; shipped: all layers of an evaluation in one launch
  // in front of the layer loop (its bitwise test: test_path_gpu.py)
  DBG_FOLD_PER_LAYER = 31,
  // (A/B, no test) smallest last round, in 256x256 tiles, that is split off as a 128x128-tile tail launch (0 = shipped: 8)
  DBG_TAIL_SPLIT_MIN = 33,
  // (A/B, no test) M-tiles per raster group of the 8-phase family (0 = shipped: 8; GemmParams.raster_gm)
  DBG_RASTER_GM = 35,
  // 1 = split-weight launches of the fp32 kernel (GEMM_FLAG_W_FLY16) on the tiles of gemm1_variant instead of fly_variant's
  // (test_x3_gpu.py, tools/fly_probe.py)
  DBG_FLY_OLD_TILES = 36,
  // 1 = x3 launches walk K' = 3K as a plain GEMM; shipped: the operand-sharing order of GEMM_FLAG_X3_SHARE.  >= 2: a class mask << 1 that
  // keeps the sharing order for those classes only (diagnosis).  (A/B through SAMAUDIO_DEBUG_FLAGS; test_x3_gpu.py compares the two walks)
  DBG_X3_PLAIN_WALK = 38,
};
// values of DBG_RESUNIT_WS: whatever the launch size (its tests; otherwise >= 1024 tiles) | never (ring kernel: A/B) | as ALWAYS on a
// grid of 3 workgroups (small cases then walk several tiles each)
enum : int { DBG_WS_ALWAYS = 1, DBG_WS_NEVER = 2, DBG_WS_ALWAYS_GRID3 = 3 };
// values of DBG_GEMM8_EPILOGUE: 0 = shipped choice (register form for 16-bit-only outputs, LDS-staged form for fp32 output / residual,
// general contract for everything else) | the general epilogue for every launch | the register / LDS form for every eligible launch (A/B)
enum : int { DBG_EPI_GENERAL = 1, DBG_EPI_LINEAR = 2, DBG_EPI_ROWS = 3 };
// values of DBG_GEMM8S_ROLES: 0 = shipped choice | none (4 waves request and multiply, round 3) | 4 requesting waves beside 4 multiplying
// ones | the same with the multiplying waves issuing 2 of their 8 loads
enum : int { DBG_ROLES_NONE = 1, DBG_ROLES_PROD0 = 2, DBG_ROLES_PROD2 = 3 };
void set_debug_flag(int flag, int value);
// SAMAUDIO_TRACE_HASH debugging aid (engine.hip): per-item checksums of a buffer; the only device allocation of the library
hipError_t launch_hash_items(const unsigned* x, size_t words_per_item, int items, unsigned long long* out, hipStream_t st);
// SAMAUDIO_OPT_SENTINEL: absmax / non-finite scan of a tensor folded into slot[0..1] (kernels.hip)
constexpr int kSentinelPartials = 256;
hipError_t launch_sentinel(const void* x, int fmt, long rows, int cols, long ld, float* partial, float* slot, hipStream_t st);
// defined (returning true) beside the real launch_sentinel only.  weak: the CPU emulation of the launchers (oracle/emu) has an empty
// launch_sentinel and no definition of this - samaudio_op_sentinel then answers SAMAUDIO_ERR_STATE instead of reporting success with
// an untouched slot, and the emulation itself stays as it is
__attribute__((weak)) bool sentinel_built();
void* debug_device_alloc(size_t bytes);
void debug_device_free(void* p);
int debug_flag(int flag);

hipError_t launch_gemm(const GemmParams& p, bool is_bf16, hipStream_t st);
const char* gemm_check(const GemmParams& p, bool is_bf16);
// Which kernel / tile shape a launch runs on.  The numbers are a debugging ABI (samaudio_debug_force_gemm_variant, the tests, the tools
// and the logs under profiles/ use them); kGemmVariantTable below has one row per id: family and profile names.
enum GemmVariant : int {
  // gemm.hip tiles (16-bit and fp32 operands)
  GV_GEMM_128x128 = 0,
  GV_GEMM_128x64 = 1,
  GV_GEMM_128x32 = 2,
  // the 16x16x32 "8-phase" family (gemm8.hip): bitwise equal between themselves
  GV_GEMM8_256x256 = 22,     // gemm8
  GV_GEMM8S_128x128 = 27,    // gemm8s: few rows; the tail of a split launch
  // the 32x32x16 family (gemm2.hip), 16-bit operands only: bitwise equal among themselves
  GV_GEMM2_128x128_S2 = 25,  // 25 / 26: 128x128 / 64x128 tiles for small M
  GV_GEMM2_64x128_S3 = 26,
  GV_GEMM2_256x64_S2 = 28,   // 64-channel convolutions
  GV_GEMM2_128x128_K32 = 29,
  GV_GEMM2_128x64_K32 = 32,
  GV_GEMM2_64x128_K32 = 33,
  GV_GEMM2_128x192_K32 = 34,
  GV_CONV7H = 35,            // k7 convolution, halo tile resident in LDS; conv7h_ok launches only
  // the fp32 kernel's 4 x 1-wave tiles of split-weight launches (gemm.hip fly_variant)
  GV_FLY_128x96 = 36,
  GV_FLY_128x128 = 37,
  GV_FLY_128x64 = 38,
  GV_FLY_128x32 = 39,
};
constexpr int kGemmVariants = 40;   // ids are < kGemmVariants
// One row per GemmVariant: the family whose accumulation order the tile shares, and its profile names for 16-bit and fp32 operands
// ("" = no such kernel).  The names are keys of the profile records and of bench.py's attribution.  (In this header, not in gemm.hip:
// engine.hip reads it too, and the CPU emulation of the launchers - oracle/emu - links engine.hip without gemm.hip.)
enum GemmFamily : int { FAM_TILES, FAM_32x32x16, FAM_8PHASE, FAM_FLY };   // gemm.hip tiles | gemm2.hip | gemm8.hip | gemm.hip fly_variant
struct GemmVariantRow {
  GemmVariant id;
  GemmFamily family;
  const char* name16;
  const char* name32;
};
inline constexpr GemmVariantRow kGemmVariantTable[] = {
    {GV_GEMM_128x128, FAM_TILES, "gemm_bf16_128x128", "gemm_f32_128x128"},
    {GV_GEMM_128x64, FAM_TILES, "gemm_bf16_128x64", "gemm_f32_128x64"},
    {GV_GEMM_128x32, FAM_TILES, "gemm_bf16_128x32", "gemm_f32_128x32"},
    {GV_GEMM8_256x256, FAM_8PHASE, "gemm8_bf16_256x256_8phase", ""},
    {GV_GEMM2_128x128_S2, FAM_32x32x16, "gemm2_bf16_128x128_s2", ""},
    {GV_GEMM2_64x128_S3, FAM_32x32x16, "gemm2_bf16_64x128_s3", ""},
    {GV_GEMM8S_128x128, FAM_8PHASE, "gemm8s_bf16_128x128", ""},
    {GV_GEMM2_256x64_S2, FAM_32x32x16, "gemm2_bf16_256x64_s2", ""},
    {GV_GEMM2_128x128_K32, FAM_32x32x16, "gemm2_bf16_128x128_k32_s3", ""},
    {GV_GEMM2_128x64_K32, FAM_32x32x16, "gemm2_bf16_128x64_k32_s2", ""},
    {GV_GEMM2_64x128_K32, FAM_32x32x16, "gemm2_bf16_64x128_k32_s3", ""},
    {GV_GEMM2_128x192_K32, FAM_32x32x16, "gemm2_bf16_128x192_k32_s3", ""},
    {GV_CONV7H, FAM_32x32x16, "conv7h_bf16", ""},
    {GV_FLY_128x96, FAM_FLY, "", "gemm_f32x3_128x96"},
    {GV_FLY_128x128, FAM_FLY, "", "gemm_f32x3_128x128"},
    {GV_FLY_128x64, FAM_FLY, "", "gemm_f32x3_128x64"},
    {GV_FLY_128x32, FAM_FLY, "", "gemm_f32x3_128x32"},
};
constexpr const GemmVariantRow* gemm_variant_row(int v) {   // nullptr: not an id
  for (const GemmVariantRow& r : kGemmVariantTable)
    if (r.id == v) return &r;
  return nullptr;
}
constexpr bool gemm_is_8phase(int v) { return gemm_variant_row(v) && gemm_variant_row(v)->family == FAM_8PHASE; }
constexpr const char* kGemm8sTailName = "gemm8s_bf16_128x128_tail";   // profile name of gemm8s as the tail of a split 8-phase GEMM
int gemm_variant(const GemmParams& p, bool is_bf16);        // the GemmVariant launch_gemm picks
const char* gemm_variant_name(int variant, bool is_bf16);   // "" for an id without a kernel of that operand type
// gemm2.hip: the 32x32x16 family's tiles; dispatches the 8-phase family and conv7h to their launchers
bool gemm2_ok(const GemmParams& p);
hipError_t launch_gemm2(const GemmParams& p, GemmVariant variant, hipStream_t st);
// gemm8.hip: 256x256 8-phase kernel (GV_GEMM8_256x256); needs gemm2_ok(p)
hipError_t launch_gemm8(const GemmParams& p, hipStream_t st);
bool gemm8_share_ok(const GemmParams& p);   // GEMM_FLAG_X3_SHARE is well-formed for this launch (gemm8.hip)
// gemm8.hip: 128x128 tile with gemm8's arithmetic (bitwise identical results), two workgroups per CU; needs gemm2_ok(p)
hipError_t launch_gemm8s(const GemmParams& p, hipStream_t st);
// gemm8.hip: GEMM_FLAG_OUT_ALT / GEMM_FLAG_OPND_ALT (mixed mode: out_act written / operands read in the alt 16-bit format) are
// well-formed; only the 8-phase family implements them
bool gemm8_alt_ok(const GemmParams& p);
// gemm8.hip: GEMM_FLAG_OUT_SPLIT3 (out_act in the compensated-operand form [lo | hi | hi]) is well-formed: launches of the 8-phase
// family with that 16-bit output only - SwiGLU, or bias + (none | GELU | quick GELU) without residual, gate or fp32 output
bool gemm8_split3_ok(const GemmParams& p);
// gemm2.hip: dilated k = 7 'same' convolution C -> C (C = 64 / 96 / 128 / 192) with the activation halo tile resident in
// LDS; bitwise equal to the implicit GEMM of the 32x32x16 family
bool conv7h_ok(const GemmParams& p);
hipError_t launch_conv7h(const GemmParams& p, hipStream_t st);
// one DAC residual unit (k7 launch p + k1 launch q on its output) as ONE kernel, bitwise equal to the two launches
bool resunit_ok(const GemmParams& p, const GemmParams& q);
hipError_t launch_resunit(const GemmParams& p, const GemmParams& q, hipStream_t st);
// gemm8.hip: one GEMM as two launches - part 0: gemm8 on the first `full` 256x256 tiles (whole rounds of the chip),
// part 1: the rest as 128x128 quadrants on gemm8s.  gemm_tail_split() = `full` for a launch (0: no split).
hipError_t launch_gemm8_split(const GemmParams& p, int full, int part, hipStream_t st);
int gemm_tail_split(const GemmParams& p, bool is_bf16);
hipError_t launch_gemm_part(const GemmParams& p, bool is_bf16, int part, hipStream_t st);
// test / tuning hook: force a variant for every eligible bf16 GEMM (-1 = automatic, 0..2 = gemm.hip tiles only,
// a GemmVariant of the 16-bit families when gemm2_ok)
void gemm_force_variant(int v);

// out[m,:] = AT( rmsnorm(x[m,:]) * w * (1 + scale) + shift ),  shift = shift_tab + tvec[b, shift_off:],
// scale likewise; b = m / rows_per_b; tvec_ld = 0 shares one conditioning row.  tvec == nullptr: no modulation.
hipError_t launch_rmsnorm_mod(const float* x, const float* w, const float* shift_tab, const float* scale_tab,
                              const float* tvec, long tvec_ld, int shift_off, int scale_off, void* out, bool bf16,
                              int M, int D, int rows_per_b, float eps, hipStream_t st);

// acc[m,:] += tanh(gate[0]) * (layernorm(x[m,:]) * w + b)
hipError_t launch_layernorm_accum(const float* x, const float* w, const float* b, const float* gate, float* acc,
                                  int M, int D, float eps, hipStream_t st);

// GroupNorm(1 group) over (T x C) per sample: partial sums, then normalise+affine+SiLU into a halo-padded
// channels-last buffer out[b][halo + t][c].
hipError_t launch_groupnorm_silu(const float* x, const float* w, const float* b, double* partials, void* out,
                                 bool bf16, int B, int T, int C, int halo, float eps, hipStream_t st);

// q/k: per-head RMSNorm (shared weight) + RoPE (adjacent pairs) -> Q,K [B,H,Tp,128]; v -> Vt [B,H,128,Tp]
// RMSNorm + modulate with pre-combined operands (kernels.hip): one launch per evaluation folds (w, shift / scale tables, the
// evaluation's shift / scale vectors) of up to kMaxModNorms norms into [norm][time value][g | s][D]
constexpr int kMaxModNorms = 96;
struct ModTables {
  const float* w[kMaxModNorms];
  const float* shift_tab[kMaxModNorms];
  const float* scale_tab[kMaxModNorms];
  int shift_off[kMaxModNorms], scale_off[kMaxModNorms];   // offsets of the norm's shift / scale inside a time vector
};
hipError_t launch_mod_tables(const ModTables& t, int n_norms, const float* tvec, long tvec_ld, int nt, float* gs, int D,
                             hipStream_t st);
hipError_t launch_rmsnorm_gs(const float* x, const float* gs, long gs_ld, void* out, bool bf16, int M, int D, int rows_per_b,
                             float eps, hipStream_t st, bool out_alt = false);   // out_alt: 16-bit output in the alt format (mixed mode)
// the same with the result in the compensated-operand form: out [M, 3D] 16-bit = [lo | hi | hi] (SAMAUDIO_OPT_X3_CLASSES)
hipError_t launch_rmsnorm_gs_split3(const float* x, const float* gs, long gs_ld, void* out, int M, int D, int rows_per_b, float eps,
                                    hipStream_t st);
hipError_t launch_qkv_prep(const void* qkv, const float* qw, const float* kw, const float* rope_cos,
                           const float* rope_sin, void* Q, void* K, void* Vt, bool bf16, int B, int T, int Tp, int H,
                           float eps, hipStream_t st, int head_dim = 128);   // head_dim 64 | 128 (rope tables [T, head_dim / 2])

// x3 contexts, head_dim 128: the same on fp32 tensors with the 16-lane-per-row access pattern of the 16-bit fast path (row statistics
// summed in another order than the general fp32 kernel: not the exact-fp32 parity mode's kernel)
hipError_t launch_qkv_prep_f32x(const float* qkv, const float* qw, const float* kw, const float* rope_cos, const float* rope_sin, float* Q,
                                float* K, float* Vt, int B, int T, int Tp, int H, float eps, hipStream_t st);

// self-attention over the padded layout above; key_mask [B,T] bytes (1 = attend); out [B*T, H*128]
hipError_t launch_self_attention(const void* Q, const void* K, const void* Vt, const unsigned char* key_mask,
                                 void* out, bool bf16, int B, int T, int Tp, int H, hipStream_t st, bool out_alt = false);

// the same with head_dim 64 or 128 (Q, K [B,H,Tp,hd], Vt [B,H,hd,Tp], out [B*T, H*hd]; scale hd^-0.5)
hipError_t launch_self_attention_hd(const void* Q, const void* K, const void* Vt, const unsigned char* key_mask,
                                    void* out, bool bf16, int B, int T, int Tp, int H, int head_dim, hipStream_t st,
                                    bool out_alt = false);

// fp32 contexts, SAMAUDIO_OPT_X3_CLASSES bit SAMAUDIO_X3_ATTENTION: the same contract on fp32 tensors with both contractions on the
// 16-bit MFMA over hi/lo-split operands (attention.hip self_attn_x3_kernel); Tp % 64 == 0
// out3 != nullptr: the context rows leave in the compensated-operand form instead, out3 [B*T, 3*H*hd] 16-bit = [lo | hi | hi]
hipError_t launch_self_attention_x3(const float* Q, const float* K, const float* Vt, const unsigned char* key_mask, float* out,
                                    int B, int T, int Tp, int H, int head_dim, hipStream_t st, void* out3 = nullptr);

// in-place per-(row, head) RMSNorm of x[rows, ld] columns [col0, col0 + H*128)
hipError_t launch_headnorm(void* x, const float* w, bool bf16, int rows, long ld, int col0, int H, float eps,
                           hipStream_t st, int head_dim = 128);

// cross attention: q [M, D] (raw, q-norm applied here), kv rows b*Lt + j with row stride kv_ld elements holding
// (k already normalised | v) in columns [0, 2D); mask [B, Lt] bytes; out [M, D]
hipError_t launch_cross_attention(const void* q, const float* qw, const void* kv, long kv_ld,
                                  const unsigned char* mask, void* out, bool bf16, int B, int T, int Lt, int H,
                                  float eps, hipStream_t st, int head_dim = 128);
// folded cross-attention output projection (bf16, Lt <= 16; see attention.hip): P [M, ldp] = softmax probabilities
// at column h*LtP + token; UT [B][D][KP] = per-batch weight operand of the GEMM h += P . U
hipError_t launch_cross_attn_probs(const void* q, const float* qw, const void* kv, long kv_ld, const unsigned char* mask,
                                   void* P, int ldp, int B, int T, int Lt, int LtP, int H, float eps, hipStream_t st);
hipError_t launch_cross_attn_fold(const void* wo, const void* kv, long kv_ld, void* UT, int KP, int B, int Lt, int LtP,
                                  int H, hipStream_t st);
// every layer of an evaluation in one launch: wo[l] = layer l's output projection, kv_all [B * Lt, kv_ld] with layer l's (k | v) in
// columns [l * 2 D, (l + 1) * 2 D), UT_all [n_layers][B][D][KP]; bitwise the per-layer launches
constexpr int kMaxFoldLayers = 48;
hipError_t launch_cross_attn_fold_layers(const void* const* wo, int n_layers, const void* kv_all, long kv_ld, void* UT_all, int KP,
                                         int B, int Lt, int LtP, int H, hipStream_t st);
// the same fold for x3 contexts (fp32 tensors in, compensated operands out; attention.hip): P3 [M, 3 KP] = [P_lo | P_hi | P_hi],
// UT3_all [n_layers][B][D][3 KP] = [U_hi | U_lo | U_hi]; q raw fp32 [M, D] (q-norm applied here), kv fp32 with k already normalised
hipError_t launch_cross_attn_probs3(const float* q, const float* qw, const float* kv, long kv_ld, const unsigned char* mask, void* P3,
                                    int KP, int B, int T, int Lt, int LtP, int H, float eps, hipStream_t st);
hipError_t launch_cross_attn_fold3_layers(const float* const* wo, int n_layers, const float* kv_all, long kv_ld, void* UT3_all, int KP,
                                          int B, int Lt, int LtP, int H, hipStream_t st);
// per-(row, layer, head) RMSNorm of the K halves of kv_all [rows, L*2D] (all layers' cross-attention keys at
// once); w_all [L, 128]
hipError_t launch_headnorm_layers(void* kv_all, const float* w_all, bool bf16, int rows, int L, int H, float eps,
                                  hipStream_t st, int head_dim = 128);

// timestep features: temb [nt, fdim] (AT) = cat(cos, sin)(t*freqs);  tsin [nt, D] fp32 likewise with inv_freq
hipError_t launch_time_features(const float* t, int nt, const float* freqs, int fdim, const float* inv_freq, int D,
                                void* temb, float* tsin, bool bf16, hipStream_t st);

// dst[0 .. n) = host_values, passed as kernel arguments (no host buffer has to outlive the call, no synchronisation)
struct FloatPack {
  static constexpr int N = 64;
  float v[N];
};
hipError_t launch_set_floats(float* dst, const float* host_values, int n, hipStream_t st);

// one combination of an explicit Runge-Kutta step (engine.hip solve_rk): out[i] = y0[i] + scale * sum_j coef[j] * k[j][i] for i < n
// (fp32, n % 4 == 0, 16-byte aligned), 1..4 sources.  `out` may be `y0` itself: the last combination of a step writes y1 over y0.
struct OdeStageArgs {
  const float* k[4];
  float coef[4];
  int n_src;
};
// weak: the CPU emulation of the launchers (oracle/emu) does not define it, and a library linked against that emulation must still
// load - ode_solve then refuses the Runge-Kutta methods (SAMAUDIO_ERR_STATE) instead of the whole library failing to bind
__attribute__((weak)) hipError_t launch_ode_stage(const float* y0, const OdeStageArgs& a, float scale, float* out, long n,
                                                  hipStream_t st);

// Adaptive solve with per-row step control (engine.hip Engine::ode_solve_adaptive).  Every row carries its own time, step
// and accept / reject decision in one OdeRowCtl on the device; all launchers below read it and only launch_ode_control writes it.
constexpr int kOdeMaxSrc = 7;      // dopri5's error estimate reads K0 .. K6
constexpr int kOdeChunk = 4096;    // elements of a row that one block of ode_error_kernel sums (a fixed tree, then one partial)
enum { ODE_ROW_RUNNING = 0, ODE_ROW_FINISHED = 1, ODE_ROW_STEP_UNDERFLOW = 2, ODE_ROW_MAX_STEPS = 3 };
struct OdeRowCtl {      // 64 bytes
  float t;              // the row's time (end of its last accepted step)
  float h;              // the trial step in flight, clipped to t1 (the stage kernels' multiplier)
  float t_new;          // t + h, or t1 exactly where the step was clipped
  float h_abs;          // the controller's proposal behind h (scipy's h_abs)
  float h_prev;         // the last accepted step
  float err;            // the last trial's error norm
  float d1, h0;         // initial-step rule: |f0 / scale|, the explicit-Euler probe step
  int status;           // ODE_ROW_*
  int accepted, rejected;
  int step_rejected;    // a trial of the current step was rejected already (caps the accept factor at 1)
  int accepted_now;     // the last decision (ode_commit_kernel's predicate)
  int n_valid;          // elements in the row's norms: valid frames * channels
  int pad[2];
};
struct OdeSrcArgs {     // up to kOdeMaxSrc device arrays [rows, row_elems] fp32 and their weights
  const float* k[kOdeMaxSrc];
  float coef[kOdeMaxSrc];
  int n_src;
};
enum { ODE_CTL_RESET = 0, ODE_CTL_INIT1 = 1, ODE_CTL_INIT2 = 2, ODE_CTL_STEP = 3 };
struct OdeControlArgs {
  float t0, t1, first_step;             // first_step <= 0: the initial-step rule (RESET leaves h = 0, INIT1 / INIT2 follow)
  float safety, ifactor, dfactor;
  int order;                            // of the error estimator (4 | 2): exponent -1 / (order + 1)
  int max_num_steps;
  int n_times;                          // rows of the time table: stages + 1
  float c[kOdeMaxSrc];                  // the table's nodes (c[0] = 0, c[n_times - 1] = 1)
};
// weak, as launch_ode_stage: the CPU emulation of the launchers has none of them and ode_solve_adaptive then answers SAMAUDIO_ERR_STATE.
// out[r, i] = y[r, i] + ctl[r].h * sum_j coef[j] k[j][r, i] for running rows, y[r, i] (no K read) for finished / failed ones;
// row_elems % 4 == 0, 16-byte aligned, out distinct from every k
__attribute__((weak)) hipError_t launch_ode_stage_rows(const float* y, const OdeSrcArgs& a, const OdeRowCtl* ctl, float* out, int rows,
                                                       long row_elems, hipStream_t st);
// partials[r, c] = sum over the valid elements i of chunk c of row r of (m * sum_j coef[j] k[j][r, i] / scale)^2 with
// scale = atol + rtol * max(|y|, |ynew|) (ynew null: |y|), m = ctl[r].h if use_h else 1; 0 for rows that are not running.  An element
// is valid iff mask[r, i / channels] != 0 (mask null: all).  partials [rows, chunks], chunks = ceil(frames * channels / kOdeChunk)
__attribute__((weak)) hipError_t launch_ode_error(const float* y, const float* ynew, const OdeSrcArgs& a, const OdeRowCtl* ctl,
                                                  const unsigned char* mask, float rtol, float atol, int use_h, float* partials, int rows,
                                                  int frames, int channels, hipStream_t st);
// one thread per row: `mode` ODE_CTL_*; sums partials (and partials_b: INIT1's second norm) in chunk order; times [n_times, rows];
// *active = rows still running afterwards
__attribute__((weak)) hipError_t launch_ode_control(OdeRowCtl* ctl, int mode, const OdeControlArgs& a, const float* partials,
                                                    const float* partials_b, int chunks, const unsigned char* mask, int frames,
                                                    int channels, float* times, int* active, int rows, hipStream_t st);
// step control per group of rows: one thread per group; groups [n_groups, 3] device i32 = first row, row
// count, row stride (null: n_groups == rows, every row its own group - launch_ode_control's arithmetic).  A group's norm adds the
// partials of its rows in window order, chunk order within a row; n_valid = the masked frames of all its rows * channels; every row
// of a group is left with the same control block and time-table column.  Row indices outside [0, rows) are skipped.
// *active = rows of the groups still running
__attribute__((weak)) hipError_t launch_ode_control_groups(OdeRowCtl* ctl, int mode, const OdeControlArgs& a, const float* partials,
                                                           const float* partials_b, int chunks, const unsigned char* mask, int frames,
                                                           int channels, float* times, int* active, int rows, const int* groups,
                                                           int n_groups, hipStream_t st);
// rows with accepted_now: y <- ynew, k_first <- k_last
__attribute__((weak)) hipError_t launch_ode_commit(float* y, const float* ynew, float* k_first, const float* k_last, const OdeRowCtl* ctl,
                                                   int rows, long row_elems, hipStream_t st);

// windowed solve of long clips (engine.hip eval_field): out [rows, W, C2] fp32 in place.  For every row r with
// next_row[r] = s in [0, rows), s != r (device i32 [rows]; anything else = no successor), every j < O and channel c:
//   p = out[r, W - O + j, c], q = out[s, j, c], v = p + a_j (q - p) with a_j = (j + 1) / (O + 1); v is written to both places.
// One lane owns both elements of a pair; 1 <= O <= W / 2 keeps the head and the tail of a row apart; C2 % 4 == 0 (float4 per lane).
// weak: the CPU emulation of the launchers (oracle/emu) does not define it - eval_field then refuses a windowed evaluation and the hook
// answers SAMAUDIO_ERR_STATE (api.hip)
__attribute__((weak)) hipError_t launch_window_blend(float* out, const int* next_row, int rows, int W, int O, int C2, hipStream_t st);

// seeded noise of separate(seed=...) (tests/noise_ref.py is the statement): out [clips * candidates, frames,
// channels] fp32, row b * candidates + c = stream (clip_ids[b], candidate c).  Quad q of frame t of a stream = one Philox4x32-10 call
// with key (seed lo, seed hi) and counter (t * channels / 4 + q, c, id lo, id hi), its four words two Box-Muller pairs: a value knows
// nothing of frames, clips, candidates or its place in the batch.  clip_ids is a HOST array: the ids travel as kernel arguments,
// NoiseClipPack::N clips per launch (values are per element, so the partition changes no bit).  channels % 4 == 0, out 16-byte
// aligned, frames * channels / 4 <= 2^32, ids >= 0: the caller's checks (api.hip).  weak: the CPU emulation of the launchers
// (oracle/emu) does not define it - the hook then answers SAMAUDIO_ERR_STATE
struct NoiseClipPack {
  static constexpr int N = 64;
  long long v[N];
};
constexpr int kNoiseGridCap = 2048;   // blocks of 256 lanes per launch; a lane walks further quads in grid strides
__attribute__((weak)) hipError_t launch_noise_rows(float* out, int clips, int candidates, int frames, int channels,
                                                   unsigned long long seed, const long long* clip_ids, hipStream_t st);

// out[r,:] = AT(x[r,:] + vec[(r / rows_per_b) * vec_ld + :])
hipError_t launch_add_rowvec(const float* x, const float* vec, long vec_ld, void* out, bool bf16, int rows, int D,
                             int rows_per_b, hipStream_t st);

// out[r,:] = AT(emb[ids[b, align[b,t]], :])   (model.py:61: embed(anchor_ids.gather(1, anchor_alignment)))
hipError_t launch_anchor_gather(const float* emb, const long* ids, int n_ids, const long* align, void* out, bool bf16,
                                int B, int T, int E, int vocab, hipStream_t st);

// generic fp32 -> AT copy with optional halo layout: out[b][halo + t][c_out_pad] <- in[b][t][c_in] (extra channels 0)
// out_bstride in elements (0 = dense (T + 2*halo) * C_out)
hipError_t launch_to_act(const float* in, long in_bstride, long in_ld, int in_col0, void* out, long out_bstride,
                         bool bf16, int B, long T, int C_in, int C_out, int halo, hipStream_t st);

// compensated 16-bit GEMM operand (SAMAUDIO_OPT_X3_CLASSES): x fp32 [M, K] (row stride ldx) -> out [M, 3K] in the library's 16-bit
// format = [lo | hi | hi] per row, hi = rn16(x), lo = rn16(x - hi); K % 8 == 0
hipError_t launch_split3(const float* x, long ldx, void* out, long M, int K, hipStream_t st);

// out[b][e] = act(in[b][e]; alpha[e % chan]) for e < count (fp32, contiguous per item, in-place allowed; count, chan % 4 == 0)
hipError_t launch_act_flat(const float* in, long in_bstride, float* out, long out_bstride, int items, long count, int chan, int act,
                           const float* alpha, hipStream_t st);

// zero the halo rows of a [B][halo + T + halo][C] buffer
hipError_t launch_zero_halo(void* buf, bool bf16, int B, long T, int C, int halo, hipStream_t st);

// ---- PE-AV transformer / Judge / span predictor (peav_kernels.hip) ------------------------------------------
// h[b][0][:] = cls; mask_s[b][0] = pad[b][0], mask_s[b][1+t] = pad[b][t]  (pad == nullptr: all valid); h is [B][T+1][D]
hipError_t launch_peav_cls_mask(float* h, const float* cls, const unsigned char* pad, unsigned char* mask_s, int B,
                                int T, int D, hipStream_t st);
// dst[b*rep + c][:] = src[b][:]
hipError_t launch_repeat_rows_u8(const unsigned char* src, unsigned char* dst, int rows, int rep, int T,
                                 hipStream_t st);
// dst[b*rep + c][:] = src[b][:], items of `elems` fp32 values (elems % 4 == 0)
hipError_t launch_repeat_items_f32(const float* src, float* dst, int items, int rep, long elems, hipStream_t st);
// masked GroupNorm(1 group) + SiLU into a halo-padded channels-last buffer; partials: B * 64 * 3 doubles
hipError_t launch_masked_groupnorm_silu(const float* x, const float* w, const float* b, const unsigned char* mask,
                                        double* partials, void* out, bool bf16, int B, int S, int C, int halo,
                                        float eps, hipStream_t st);
// the same with the result as a compensated GEMM operand (SAMAUDIO_OPT_X3_CLASSES): out3 [B][S + 2 halo][3C] 16-bit, valid frames
// [lo | hi | hi] of the fp32 kernel's value, masked frames zeros, halo rows untouched.  weak: the CPU emulation of the launchers
// (oracle/emu) does not define it - the x3 towers then write the fp32 buffer and split it with launch_split3 (peav.hip)
__attribute__((weak)) hipError_t launch_masked_groupnorm_silu_split3(const float* x, const float* w, const float* b,
                                                                     const unsigned char* mask, double* partials, void* out3, int B,
                                                                     int S, int C, int halo, float eps, hipStream_t st);
// out[m,:] = LayerNorm(x[m,:]) * w + b; either output may be null
hipError_t launch_layernorm_rows(const float* x, long x_ld, const float* w, const float* b, float* out_f32,
                                 void* out_act, bool bf16, long M, int D, float eps, hipStream_t st);
// the same with the result as a compensated GEMM operand (SAMAUDIO_OPT_X3_CLASSES): out3 [M, 3D] 16-bit = [lo | hi | hi] of the fp32
// value - the bits of launch_layernorm_rows(..., out_f32) followed by launch_split3; D <= 2048.  weak: the CPU emulation of the
// launchers (oracle/emu) does not define it - the parity hook then answers SAMAUDIO_ERR_STATE (api.hip)
__attribute__((weak)) hipError_t launch_layernorm_rows_split3(const float* x, long x_ld, const float* w, const float* b, void* out3,
                                                              long M, int D, float eps, hipStream_t st);
// scores[b][j] = (masked mean over frames of hidden[b][1+t][:]) . head_w[j][:] * std[j] + mean[j]
hipError_t launch_judge_pool_head(const float* hidden, const unsigned char* mask_s, const float* head_w,
                                  const float* mean, const float* std_, float* out, int B, int T, int D,
                                  hipStream_t st);
// logits[b][t] = <audio[a_off + b*a_bstride + t*E + :], text[b][:]> * scale[0] + bias[0]
hipError_t launch_frame_logits(const float* audio, long a_bstride, long a_off, const float* text, const float* scale,
                               const float* bias, float* out, int B, int T, int E, hipStream_t st);

// ---- audio front end (kernels.hip) -------------------------------------------------------------------------------
// One PCM clip (int16 scaled by 1 / 32768 | fp32; element (c, i) at pcm[c * ch_stride + i * s_stride]) -> out[0, out_len) = the mean
// over the channels resampled by the compact polyphase bank of samaudio.h (taps [K][phases] tap-major, first [phases]; `step` input
// samples per `phases` outputs), out[out_len, out_capacity) = 0.  weak: the CPU emulation of the launchers (oracle/emu) does not
// define it - the hook then answers SAMAUDIO_ERR_STATE (api.hip)
__attribute__((weak)) hipError_t launch_resample_mix(const void* pcm, bool s16, int channels, long samples, long ch_stride,
                                                     long s_stride, const float* taps, const int* first, int phases, int step, int K,
                                                     float* out, long out_len, long out_capacity, hipStream_t st);

// ---- sound activity (kernels.hip) --------------------------------------------------------------------------------
// `rows` mono fp32 waveforms (row r at wav + r * row_stride) -> int16 -> 24 kHz (`step` input samples per `phases` frames, phases a
// divisor of 24 000; N frames, L ms: samaudio.h) -> cells [rows][L] i64 (the workspace: sums of y^2 per millisecond) -> per row the
// nonsilent spans in ms (spans [rows][max_spans][2], span_count [rows], peak [rows]: each may be null) and scores [rows] = iou | recall | precision (metric 0 | 1 | 2) against ref_spans [n_ref][2] f64 seconds (null = none: score 0).
// Two launches.  weak: the CPU emulation of the launchers (oracle/emu) does not define it - the hook then answers SAMAUDIO_ERR_STATE
__attribute__((weak)) hipError_t launch_activity(const float* wav, int rows, long row_stride, int step, int phases, long N, long L,
                                                 const int* table, const double* ref_spans, int n_ref, int metric, long long* cells,
                                                 float* scores, int* spans, int max_spans, int* span_count, int* peak,
                                                 hipStream_t st);

// ---- CLAP log-mel front end (kernels.hip) -------------------------------------------------------------------------
// `rows` mono fp32 waveforms of one length n (row r at wav + r * row_stride) -> out [rows][frames][n_mels] dB features: the int16 round
// trip (quantise), repeatpad to L / the crop [offset, offset + L), centred reflect-padded frames of N = 1 << log2n samples at `hop`,
// window, real FFT in LDS, |X|^2, the mel bank [N / 2 + 1][n_mels], 10 log10(max(., 1e-10)), the per-mel scale and shift (null = none):
// samaudio.h samaudio_op_logmel.  tables = window [N] | (cos, -sin)(2 pi t / N) [N / 2][2].  One launch.  weak: the CPU emulation of
// the launchers (oracle/emu) does not define it - the hook then answers SAMAUDIO_ERR_STATE
__attribute__((weak)) hipError_t launch_clap_logmel(const float* wav, int rows, long row_stride, long n, long offset, int L, bool quantise,
                                                    int log2n, int hop, int n_mels, int frames, const float* tables, const float* bank,
                                                    const float* bn_scale, const float* bn_shift, float* out, hipStream_t st);

// ---- CLAP towers (clap_kernels.hip; samaudio.h "CLAP ranker towers").  fp32 only.  weak: the CPU builds of the launchers under oracle/
// do not define them - the hooks and the tower then answer SAMAUDIO_ERR_STATE ----------------------------------------
// feat [n][frames][F] (normalised log-mel) -> tokens [n][G * G][C], G = spec / stride: bicubic align_corners time interpolation to
// spec * (spec / F) frames where frames is below that, the mel-to-image fold (image row r F + f, column x = frame r spec + x), the
// P x P stride-S convolution (w [C][P * P], padding (P - S) / 2, bias), LayerNorm(C) (ln_w null = none).  C <= 1024, P * P <= 64
__attribute__((weak)) hipError_t launch_clap_patch_embed(const float* feat, int n, int frames, int F, int spec, int P, int S, int C,
                                                         const float* w, const float* bias, const float* ln_w, const float* ln_b,
                                                         float eps, float* tokens, hipStream_t st);
// shifted-window attention on q|k|v rows [n * H * W][3 * heads * hd]: per (clip, window, head) the ws x ws tokens at the rolled,
// window-partitioned positions, softmax(q k^T / sqrt(hd) + table[rel(i, j)][head] + region mask (-100, shift > 0 only)) v, written to
// out [n * H * W][heads * hd] at the un-rolled positions.  hd 24 | 32, ws * ws <= 64, H % ws == W % ws == 0, table [(2 ws - 1)^2][heads]
__attribute__((weak)) hipError_t launch_swin_window_attn(const float* qkv, const float* table, float* out, int n, int H, int W,
                                                         int heads, int hd, int ws, int shift, hipStream_t st);
// x [n][H * W][C] -> out [n][H/2 * W/2][4 C] = LayerNorm(4 C) of (x(2y, 2x) | x(2y + 1, 2x) | x(2y, 2x + 1) | x(2y + 1, 2x + 1))
__attribute__((weak)) hipError_t launch_swin_patch_merge(const float* x, const float* ln_w, const float* ln_b, float eps, float* out,
                                                         int n, int H, int W, int C, hipStream_t st);
// RoBERTa embeddings before their LayerNorm: out[r][t] = word[ids] + pos[position] + type[0], position = pad + (number of non-pad ids
// in row r up to and including t) for a non-pad id, pad for a pad id (modeling_clap.py:1010).  T <= 1024
__attribute__((weak)) hipError_t launch_clap_text_embed(const long long* ids, const float* word, const float* pos, const float* type,
                                                        float* out, int rows, int T, int D, int vocab, int pad, hipStream_t st);
// scores[b][c] = <audio[b * cand + c][:], text[b][:]> (one wave per score, a fixed summation order)
__attribute__((weak)) hipError_t launch_clap_score(const float* audio, const float* text, float* scores, int clips, int cand, int dim,
                                                   hipStream_t st);

// ---- PE-Core vision tower (vit_kernels.hip) ---------------------------------------------------------------------
// im2col of the k = stride = P patch convolution: frames [n,3,S,S] f32 -> rows [n*(S/P)^2, Kp], column c*P*P + py*P + px
hipError_t launch_patchify(const float* frames, void* out, bool bf16, int n, int S, int P, int Kp, hipStream_t st);
// uint8 frames [n,3,H,W] -> S x S (mode = SAMAUDIO_RESIZE_*: nearest | antialiased bilinear | antialiased bicubic), rounded half to
// even, clamped to 0..255, (v / 255 - 0.5) / 0.5.  Kp == 0: planar f32 [n,3,S,S] (bf16 false).  Kp > 0: launch_patchify's rows of
// that image, [n*(S/P)^2, Kp] in the operand type.  weak: the CPU emulation of the launchers (oracle/emu) does not define it - the
// parity hook then answers SAMAUDIO_ERR_STATE (api.hip)
__attribute__((weak)) hipError_t launch_resize_frames(const unsigned char* frames, int n, int H, int W, int S, int mode, void* out,
                                                      bool bf16, int P, int Kp, hipStream_t st);
// launch_resize_frames on n frames picked from a video [src_frames,3,H,W]: output frame f from source frame pick[f] (device i32 [n];
// null = f, n == src_frames; values are clamped into the video), source pixels whose byte of mask [src_frames,mc,H,W] (mc = 1 | 3;
// null = no mask) is non-zero count as 0.  Bit-identical to launch_resize_frames on (frames * (mask == 0))[pick].  weak: as above
__attribute__((weak)) hipError_t launch_resize_video(const unsigned char* frames, long src_frames, int H, int W,
                                                     const unsigned char* mask, int mc, const int* pick, int n, int S, int mode,
                                                     void* out, bool bf16, int P, int Kp, hipStream_t st);
// q|k|v rows [n*T, 3*H*hd] -> Q, K [n,H,Tp,hd] (adjacent-pair rotation by rc / rs [T, hd/2]; null = none), V^T [n,H,hd,Tp]
// (the four below are weak: the CPU emulation of the launchers - oracle/emu - links api.hip without vit_kernels.hip, and their parity
// hooks then answer SAMAUDIO_ERR_STATE)
__attribute__((weak)) hipError_t launch_rope2d_split(const void* qkv, const float* rc, const float* rs, void* Q, void* K, void* Vt,
                                                     bool bf16, int n, int T, int Tp, int H, int head_dim, hipStream_t st);
// one query per head over all tokens: q [H*hd] f32, kv rows [n*T, 2*H*hd] = (k | v) -> out [n, H*hd]
__attribute__((weak)) hipError_t launch_pool_attention(const float* q, const void* kv, void* out, bool bf16, int n, int T, int H,
                                                       int head_dim, hipStream_t st);
__attribute__((weak)) hipError_t launch_l2_normalize(float* x, int rows, int D, hipStream_t st);
// out[f, :] = mean over the T tokens of x[f, t, :]
__attribute__((weak)) hipError_t launch_token_mean(const float* x, long x_ld, float* out_f32, void* out_act, bool bf16, int n, int T,
                                                   int D, hipStream_t st);

// ---- T5 prompt encoder (t5_kernels.hip) ------------------------------------------------------------
// out[m, :] = table[ids[m], :], ids clamped into [0, vocab); D % 4 == 0.  weak: oracle/emu links api.hip without t5_kernels.hip; the
// parity hook samaudio_op_embed_rows then answers SAMAUDIO_ERR_STATE
__attribute__((weak)) hipError_t launch_t5_embed(const long long* ids, const float* table, float* out, long M, int D, int vocab,
                                                 hipStream_t st);
// softmax(q k^T + bias[h][k - q] + key mask) v per (item, head, query row); qkv [B*Lt, 3*H*dkv]; Lt <= 512, dkv <= 128
// (bias nullable; scale multiplies q k^T; window > 0: only keys within +-window tokens)
// (this one and the two below are weak: oracle/emu links api.hip without t5_kernels.hip; their parity hooks then answer
// SAMAUDIO_ERR_STATE)
__attribute__((weak)) hipError_t launch_t5_attention(const void* qkv, const unsigned char* mask, const float* bias, void* out, bool bf16,
                                                     int B, int Lt, int H, int dkv, int max_len, float scale, int window,
                                                     hipStream_t st);
// ModernBERT text tower (mbert.hip): rotate-half RoPE of the q / k segments of q|k|v rows in place; gated GELU
__attribute__((weak)) hipError_t launch_mbert_rope(void* qkv, const float* cs, const float* sn, bool bf16, long M, int Lt, int H, int hd,
                                                   hipStream_t st);
__attribute__((weak)) hipError_t launch_geglu(const void* x, void* out, bool bf16, long M, int F, hipStream_t st);

}  // namespace sa
