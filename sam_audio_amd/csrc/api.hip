// extern "C" surface of libsamaudio_hip.so (declared in include/samaudio.h).
#include <cstring>
#include <string>

#include "engine.h"
#include "peav.h"

struct samaudio_ctx {
  sa::Engine* engine;
};
struct samaudio_judge {
  sa::Judge* judge;
};
struct samaudio_frame {
  sa::FramePredictor* frame;
};

namespace {
thread_local std::string g_err;
}  // namespace
namespace sa {
void set_last_error(const std::string& msg) { g_err = msg; }  // for the C entry points that live in other files (vit.hip)
}  // namespace sa
namespace {
int hip_ret(hipError_t e, const char* what) {
  if (e == hipSuccess) return SAMAUDIO_OK;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return SAMAUDIO_ERR_HIP;
}
using sa::bad;
using sa::ret;
}  // namespace

extern "C" {

const char* samaudio_last_error(void) { return g_err.c_str(); }
#ifdef SA_OPERAND_FP16
const char* samaudio_version(void) { return "samaudio-hip 0.1 (gfx950, fp16 operands)"; }
#else
const char* samaudio_version(void) { return "samaudio-hip 0.1 (gfx950)"; }
#endif

int samaudio_create(const samaudio_config* cfg, samaudio_ctx** out) {
  if (!cfg || !out) return bad("samaudio_create: null argument");
  if (cfg->precision != SAMAUDIO_F32 && cfg->precision != SAMAUDIO_BF16) return bad("samaudio_create: precision");
  if (cfg->dim <= 0 || cfg->n_heads <= 0 || cfg->n_layers < 0 || cfg->ffn_hidden <= 0) return bad("samaudio_create: dims");
  samaudio_ctx* c = new samaudio_ctx;
  c->engine = new sa::Engine(*cfg);
  *out = c;
  return SAMAUDIO_OK;
}

void samaudio_destroy(samaudio_ctx* ctx) {
  if (!ctx) return;
  delete ctx->engine;
  delete ctx;
}

int samaudio_set_tensor(samaudio_ctx* ctx, const char* name, const void* data, int dtype, int ndim,
                        const int64_t* shape) {
  return SA_ENTRY(ctx, "null context", ctx->engine->set_tensor(name, data, dtype, ndim, shape));
}

int samaudio_set_option(samaudio_ctx* ctx, int option, int value) {
  return SA_ENTRY(ctx, "null context", ctx->engine->set_option(option, value));
}

int samaudio_finalize(samaudio_ctx* ctx, int what) {
  return SA_ENTRY(ctx, "null context", ctx->engine->finalize(what));
}

size_t samaudio_workspace_bytes(samaudio_ctx* ctx, int rows, int frames, int text_len, int codec_items,
                                int64_t samples) {
  if (!ctx) return 0;
  return ctx->engine->workspace_bytes(rows, frames, text_len, codec_items, samples);
}

int samaudio_set_workspace(samaudio_ctx* ctx, void* workspace, size_t bytes) {
  return SA_ENTRY(ctx, "null context", ctx->engine->set_workspace(workspace, bytes));
}

int samaudio_prepare(samaudio_ctx* ctx, int rows, int frames, int text_len, const float* audio_features,
                     const float* text, const uint8_t* text_mask, const float* video, const int64_t* anchor_ids,
                     int n_ids, const int64_t* anchor_alignment, const uint8_t* audio_pad_mask,
                     samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context",
                  ctx->engine->prepare(rows, frames, text_len, audio_features, text, text_mask, video, anchor_ids, n_ids,
                      anchor_alignment, audio_pad_mask, (hipStream_t)stream));
}

int samaudio_prepare_latent(samaudio_ctx* ctx, int rows, int frames, int text_len, int candidates, const float* latent,
                            const float* text, const uint8_t* text_mask, const float* video, const int64_t* anchor_ids,
                            int n_ids, const int64_t* anchor_alignment, const uint8_t* audio_pad_mask, samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context",
                  ctx->engine->prepare(rows, frames, text_len, latent, text, text_mask, video, anchor_ids, n_ids,
                      anchor_alignment, audio_pad_mask, (hipStream_t)stream, candidates, true));
}

int samaudio_forward(samaudio_ctx* ctx, const float* noisy, const float* time, int n_time, float* out,
                     samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->forward(noisy, time, n_time, out, (hipStream_t)stream));
}

int samaudio_ode_solve(samaudio_ctx* ctx, float* state, int method, const float* grid_host, int n_grid,
                       samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->ode_solve(state, method, grid_host, n_grid, (hipStream_t)stream));
}

int samaudio_ode_solve_adaptive(samaudio_ctx* ctx, float* state, int method, float t0, float t1, const samaudio_ode_adaptive* opt,
                                samaudio_ode_row_stats* stats_host, samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->ode_solve_adaptive(state, method, t0, t1, opt, stats_host, (hipStream_t)stream));
}

size_t samaudio_ode_stage_bytes(samaudio_ctx* ctx, int method, int rows, int frames) {
  if (!ctx) return 0;
  return ctx->engine->ode_stage_bytes(method, rows, frames);
}

int samaudio_set_ode_stages(samaudio_ctx* ctx, void* stages, size_t bytes) {
  return SA_ENTRY(ctx, "null context", ctx->engine->set_ode_stages(stages, bytes));
}

int samaudio_set_windows(samaudio_ctx* ctx, const int32_t* next_row_device, int rows, int overlap_frames) {
  return SA_ENTRY(ctx, "null context", ctx->engine->set_windows(next_row_device, rows, overlap_frames));
}

int samaudio_set_window_groups(samaudio_ctx* ctx, const int32_t* groups_device, int n_groups, const uint8_t* owner_mask_device) {
  return SA_ENTRY(ctx, "null context", ctx->engine->set_window_groups(groups_device, n_groups, owner_mask_device));
}

int samaudio_codec_encode(samaudio_ctx* ctx, const float* wav, int items, int64_t samples, float* latent,
                          samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->codec_encode(wav, items, samples, latent, (hipStream_t)stream));
}

int samaudio_codec_decode(samaudio_ctx* ctx, const float* latent, int items, int frames, float* wav,
                          samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->codec_decode(latent, items, frames, wav, (hipStream_t)stream));
}

int samaudio_codec_decode_pairs(samaudio_ctx* ctx, const float* state, int rows, int frames, float* wav, samaudio_stream stream) {
  if (!ctx) return bad("null context");
  if (rows <= 0) return bad("codec_decode_pairs: rows");
  return ret(ctx->engine->codec_decode(state, 2 * rows, frames, wav, (hipStream_t)stream, true));
}

int samaudio_codec_halo_frames(samaudio_ctx* ctx, int decode) { return ctx ? ctx->engine->codec_halo_frames(decode != 0) : -1; }

int64_t samaudio_codec_tile_samples(samaudio_ctx* ctx, int frames, int tile_frames, int decode) {
  return ctx ? ctx->engine->codec_tile_samples(frames, tile_frames, decode != 0) : -1;
}

int samaudio_codec_encode_tiled(samaudio_ctx* ctx, const float* wav, int items, int64_t samples, int tile_frames, float* latent,
                                samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->codec_encode_tiled(wav, items, samples, tile_frames, latent, (hipStream_t)stream));
}

int samaudio_codec_decode_tiled(samaudio_ctx* ctx, const float* latent, int items, int frames, int tile_frames, float* wav,
                                samaudio_stream stream) {
  return SA_ENTRY(ctx, "null context", ctx->engine->codec_decode_tiled(latent, items, frames, tile_frames, wav, (hipStream_t)stream));
}

int samaudio_codec_decode_pairs_tiled(samaudio_ctx* ctx, const float* state, int rows, int frames, int tile_frames, float* wav,
                                      samaudio_stream stream) {
  if (!ctx) return bad("null context");
  if (rows <= 0) return bad("codec_decode_pairs_tiled: rows");
  return ret(ctx->engine->codec_decode_tiled(state, 2 * rows, frames, tile_frames, wav, (hipStream_t)stream, true));
}

void samaudio_debug_force_gemm_variant(int variant) { sa::gemm_force_variant(variant); }
void samaudio_debug_set_flag(int flag, int value) { sa::set_debug_flag(flag, value); }
int samaudio_debug_poison_lds(samaudio_stream stream) {
  return hip_ret(sa::launch_poison_lds((hipStream_t)stream), "poison_lds");
}

int samaudio_profile_begin(samaudio_ctx* ctx) {
  return SA_ENTRY(ctx, "null context", ctx->engine->profile_begin());
}

int samaudio_sentinel_read(samaudio_ctx* ctx, float* absmax, double* nonfinite, samaudio_stream stream) {
  if (!ctx || !absmax || !nonfinite) return bad("samaudio_sentinel_read: null argument");
  return ret(ctx->engine->sentinel_read(absmax, nonfinite, (hipStream_t)stream));
}


int samaudio_profile_end(samaudio_ctx* ctx, samaudio_kernel_stat* out, int capacity, int* count) {
  if (!ctx || !count || (capacity > 0 && !out)) return bad("samaudio_profile_end: null argument");
  std::vector<sa::Engine::KernelStat> st;
  const int rc = ret(ctx->engine->profile_end(st));
  if (rc) return rc;
  int n = 0;
  for (const auto& k : st) {
    if (k.launches == 0) continue;
    if (n >= capacity) break;
    std::memset(&out[n], 0, sizeof(out[n]));
    std::strncpy(out[n].name, k.name.c_str(), sizeof(out[n].name) - 1);
    out[n].launches = k.launches;
    out[n].flops = k.flops;
    out[n].bytes = k.bytes;
    out[n].ms = k.ms;
    ++n;
  }
  *count = n;
  return SAMAUDIO_OK;
}

// ---- per-kernel hooks ------------------------------------------------------------------------------
int samaudio_op_gemm(const void* params_host, size_t params_bytes, int precision, samaudio_stream stream) {
  if (!params_host || params_bytes != sizeof(sa::GemmParams)) return bad("samaudio_op_gemm: GemmParams size mismatch");
  sa::GemmParams p;
  std::memcpy(&p, params_host, sizeof(p));
  const bool bf16 = precision == SAMAUDIO_BF16;
  if (const char* why = sa::gemm_check(p, bf16)) return bad(why);
  return hip_ret(sa::launch_gemm(p, bf16, (hipStream_t)stream), "gemm");
}

int samaudio_op_codec_conv(const void* params_host, size_t params_bytes, const void* w_twin, int twin_kind, int cin, void* scratch,
                           size_t scratch_bytes, int* path, samaudio_stream stream) {
  if (!params_host || params_bytes != sizeof(sa::GemmParams)) return bad("samaudio_op_codec_conv: GemmParams size mismatch");
  if (twin_kind < SAMAUDIO_CODEC_TWIN_NONE || twin_kind > SAMAUDIO_CODEC_TWIN_X3 || (twin_kind != SAMAUDIO_CODEC_TWIN_NONE && !w_twin))
    return bad("samaudio_op_codec_conv: twin_kind / w_twin");
  sa::GemmParams p_in;
  std::memcpy(&p_in, params_host, sizeof(p_in));
  hipStream_t st = (hipStream_t)stream;
  // what Engine::codec_gemm does in an fp32 context with class CODEC on compensated operands, by the same functions of host.h
  const bool wide = twin_kind == SAMAUDIO_CODEC_TWIN_X3 && scratch && sa::codec_x3_eligible(p_in, cin, scratch_bytes);
  if (!wide) {
    sa::GemmParams p = sa::gemm_launch_params(p_in, 1, true, false, -1);
    sa::codec_fly_operands(p, twin_kind == SAMAUDIO_CODEC_TWIN_FLY ? w_twin : nullptr);
    if (path) *path = SAMAUDIO_CODEC_PATH_FLY;
    if (const char* why = sa::gemm_check(p, false)) return bad(why);
    return hip_ret(sa::launch_gemm(p, false, st), "codec_conv");
  }
  const bool whole_k = sa::codec_x3_whole_k(p_in, cin);
  if (path) *path = whole_k ? SAMAUDIO_CODEC_PATH_X3 : SAMAUDIO_CODEC_PATH_X3_BLOCK;
  if (hipError_t e = sa::launch_split3((const float*)p_in.A, cin, scratch, sa::codec_x3_split_rows(p_in, cin), cin, st); e != hipSuccess)
    return hip_ret(e, "codec_conv: split3");
  const sa::GemmParams p = sa::gemm_launch_params(sa::codec_x3_launch(p_in, scratch, w_twin), 1, true, false,
                                                  whole_k ? SAMAUDIO_CLS_CODEC : -1);
  if (const char* why = sa::gemm_check(p, true)) return bad(why);
  if (hipError_t e = sa::launch_gemm(p, true, st); e != hipSuccess) return hip_ret(e, "codec_conv: gemm");
  const sa::CodecActPass a = sa::codec_x3_act(p_in);
  if (!a.run) return SAMAUDIO_OK;
  if (!a.aligned) return bad("samaudio_op_codec_conv: window start is not a whole channel row");
  return hip_ret(sa::launch_act_flat(a.in, a.in_bstride, a.out, a.out_bstride, a.items, a.count, a.chan, a.act, a.alpha, st),
                 "codec_conv: act");
}

int samaudio_op_resunit(const void* conv7_params_host, const void* conv1_params_host, size_t params_bytes,
                        samaudio_stream stream) {
  if (!conv7_params_host || !conv1_params_host || params_bytes != sizeof(sa::GemmParams))
    return bad("samaudio_op_resunit: GemmParams size mismatch");
  sa::GemmParams p, q;
  std::memcpy(&p, conv7_params_host, sizeof(p));
  std::memcpy(&q, conv1_params_host, sizeof(q));
  if (const char* why = sa::gemm_check(p, true)) return bad(why);
  if (const char* why = sa::gemm_check(q, true)) return bad(why);
  if (!sa::resunit_ok(p, q)) return bad("samaudio_op_resunit: not a (k7, k1) residual-unit pair the fused kernel covers");
  return hip_ret(sa::launch_resunit(p, q, (hipStream_t)stream), "resunit");
}

// ---- the norm hooks (tests/test_norm_kernels_gpu.py): they refuse what their kernels assume, then call the launcher unchanged ----
namespace {
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool al_out(const void* p, int precision) { return ((uintptr_t)p & (precision == SAMAUDIO_BF16 ? 7 : 15)) == 0; }
}  // namespace

int samaudio_op_rmsnorm_mod(const float* x, const float* w, const float* shift_tab, const float* scale_tab,
                            const float* tvec, int64_t tvec_ld, int shift_off, int scale_off, void* out,
                            int precision, int rows, int dim, int rows_per_batch, float eps, samaudio_stream stream) {
  if (!x || !w || !out) return bad("rmsnorm_mod: null x / w / out");
  if (rows <= 0) return bad("rmsnorm_mod: rows <= 0");
  if (dim <= 0 || dim % 4) return bad("rmsnorm_mod: dim % 4 (and dim > 0)");
  if (rows_per_batch <= 0) return bad("rmsnorm_mod: rows_per_batch <= 0");
  const int given = (shift_tab ? 1 : 0) + (scale_tab ? 1 : 0) + (tvec ? 1 : 0);
  if (given != 0 && given != 3) return bad("rmsnorm_mod: shift_tab, scale_tab and tvec are given together or not at all");
  if (tvec) {
    if (tvec_ld < 0 || tvec_ld % 4) return bad("rmsnorm_mod: tvec_ld % 4");
    if (shift_off < 0 || shift_off % 4) return bad("rmsnorm_mod: shift_off % 4");
    if (scale_off < 0 || scale_off % 4) return bad("rmsnorm_mod: scale_off % 4");
  }
  if (!al16(x) || !al16(w) || !al16(shift_tab) || !al16(scale_tab) || !al16(tvec) || !al_out(out, precision))
    return bad("rmsnorm_mod: x, w, shift_tab, scale_tab and tvec must be aligned to 16 bytes, out to 16 (fp32) / 8 (16-bit)");
  return hip_ret(sa::launch_rmsnorm_mod(x, w, shift_tab, scale_tab, tvec, tvec_ld, shift_off, scale_off, out,
                                        precision == SAMAUDIO_BF16, rows, dim, rows_per_batch, eps,
                                        (hipStream_t)stream), "rmsnorm_mod");
}

int samaudio_op_groupnorm_silu(const float* x, const float* w, const float* b, void* partials_f64, void* out,
                               int precision, int batch, int frames, int channels, int halo, float eps,
                               samaudio_stream stream) {
  if (!x || !w || !b || !partials_f64 || !out) return bad("groupnorm: null x / w / b / partials_f64 / out");
  if (batch <= 0) return bad("groupnorm: batch <= 0");
  if (frames <= 0) return bad("groupnorm: frames <= 0");
  if (channels <= 0 || channels % 4) return bad("groupnorm: channels % 4 (and channels > 0)");
  if (halo < 0) return bad("groupnorm: halo < 0");
  if (!al16(x) || !al16(w) || !al16(b) || ((uintptr_t)partials_f64 & 7) || !al_out(out, precision))
    return bad("groupnorm: x, w and b must be aligned to 16 bytes, partials_f64 to 8, out to 16 (fp32) / 8 (16-bit)");
  return hip_ret(sa::launch_groupnorm_silu(x, w, b, (double*)partials_f64, out, precision == SAMAUDIO_BF16, batch,
                                           frames, channels, halo, eps, (hipStream_t)stream), "groupnorm_silu");
}

int samaudio_op_qkv_prep(const void* qkv, const float* q_w, const float* k_w, const float* rope_cos,
                         const float* rope_sin, void* q, void* k, void* vt, int precision, int batch, int frames,
                         int frames_padded, int heads, float eps, samaudio_stream stream) {
  if (frames_padded % 64 || frames_padded < frames) return bad("qkv_prep: frames_padded");
  return hip_ret(sa::launch_qkv_prep(qkv, q_w, k_w, rope_cos, rope_sin, q, k, vt, precision == SAMAUDIO_BF16, batch,
                                     frames, frames_padded, heads, eps, (hipStream_t)stream), "qkv_prep");
}

int samaudio_op_self_attention(const void* q, const void* k, const void* vt, const uint8_t* key_mask, void* out,
                               int precision, int batch, int frames, int frames_padded, int heads,
                               samaudio_stream stream) {
  if (frames_padded % 64 || frames_padded < frames) return bad("self_attention: frames_padded");
  if (precision == 2)   // fp32 tensors, both contractions on hi/lo-split operands (SAMAUDIO_X3_ATTENTION)
    return hip_ret(sa::launch_self_attention_x3((const float*)q, (const float*)k, (const float*)vt, key_mask, (float*)out, batch, frames,
                                                frames_padded, heads, 128, (hipStream_t)stream), "self_attention_x3");
  return hip_ret(sa::launch_self_attention(q, k, vt, key_mask, out, precision == SAMAUDIO_BF16, batch, frames,
                                           frames_padded, heads, (hipStream_t)stream), "self_attention");
}

int samaudio_op_cross_attention(const void* q, const float* q_w, void* kv, const float* k_w, const uint8_t* mask,
                                void* out, int precision, int batch, int frames, int text_len, int heads, float eps,
                                samaudio_stream stream) {
  const bool bf16 = precision == SAMAUDIO_BF16;
  hipError_t e = sa::launch_headnorm(kv, k_w, bf16, batch * text_len, 2L * heads * 128, 0, heads, eps,
                                     (hipStream_t)stream);
  if (e != hipSuccess) return hip_ret(e, "headnorm");
  return hip_ret(sa::launch_cross_attention(q, q_w, kv, 2L * heads * 128, mask, out, bf16, batch, frames, text_len, heads, eps,
                                            (hipStream_t)stream), "cross_attention");
}

int samaudio_op_cross_attn_fold(const void* wo, const void* kv, int64_t kv_ld, void* ut, int kp, int batch, int text_len,
                                int ltp, int heads, samaudio_stream stream) {
  if (text_len > 16 || (ltp != 8 && ltp != 16) || kp % 64 || kp < heads * ltp) return bad("cross_attn_fold: shape");
  return hip_ret(sa::launch_cross_attn_fold(wo, kv, kv_ld, ut, kp, batch, text_len, ltp, heads, (hipStream_t)stream),
                 "cross_attn_fold");
}

int samaudio_op_layernorm_accum(const float* x, const float* w, const float* b, const float* gate, float* acc,
                                int rows, int dim, float eps, samaudio_stream stream) {
  if (!x || !w || !b || !gate || !acc) return bad("layernorm_accum: null x / w / b / gate / acc");
  if (rows <= 0) return bad("layernorm_accum: rows <= 0");
  if (dim <= 0 || dim % 4) return bad("layernorm_accum: dim % 4 (and dim > 0)");
  if (!al16(x) || !al16(w) || !al16(b) || !al16(acc)) return bad("layernorm_accum: x, w, b and acc must be aligned to 16 bytes");
  return hip_ret(sa::launch_layernorm_accum(x, w, b, gate, acc, rows, dim, eps, (hipStream_t)stream),
                 "layernorm_accum");
}

int samaudio_op_masked_groupnorm_silu(const float* x, const float* w, const float* b, const uint8_t* mask,
                                      void* partials_f64, void* out, int precision, int batch, int frames,
                                      int channels, int halo, float eps, samaudio_stream stream) {
  if (!x || !w || !b || !mask || !partials_f64 || !out) return bad("masked_groupnorm: null x / w / b / mask / partials_f64 / out");
  if (batch <= 0) return bad("masked_groupnorm: batch <= 0");
  if (frames <= 0) return bad("masked_groupnorm: frames <= 0");
  if (channels <= 0 || channels % 4) return bad("masked_groupnorm: channels % 4 (and channels > 0)");
  if (halo < 0) return bad("masked_groupnorm: halo < 0");
  if (!al16(x) || !al16(w) || !al16(b) || ((uintptr_t)partials_f64 & 7) || !al_out(out, precision))
    return bad("masked_groupnorm: x, w and b must be aligned to 16 bytes, partials_f64 to 8, out to 16 (fp32) / 8 (16-bit)");
  return hip_ret(sa::launch_masked_groupnorm_silu(x, w, b, mask, (double*)partials_f64, out, precision == SAMAUDIO_BF16,
                                                  batch, frames, channels, halo, eps, (hipStream_t)stream),
                 "masked_groupnorm_silu");
}

int samaudio_op_masked_groupnorm_silu_split3(const float* x, const float* w, const float* b, const uint8_t* mask,
                                             void* partials_f64, void* out3, int batch, int frames, int channels, int halo,
                                             float eps, samaudio_stream stream) {
  if (channels % 4 || !mask || !x || !w || !b || !out3 || !partials_f64 || batch <= 0 || frames <= 0 || halo < 0)
    return bad("masked_groupnorm_split3: channels % 4 / null argument");
  if (!sa::launch_masked_groupnorm_silu_split3) return bad("masked_groupnorm_split3: not in this build of the library");
  return hip_ret(sa::launch_masked_groupnorm_silu_split3(x, w, b, mask, (double*)partials_f64, out3, batch, frames, channels, halo,
                                                         eps, (hipStream_t)stream),
                 "masked_groupnorm_silu_split3");
}

int samaudio_op_layernorm_rows(const float* x, int64_t x_ld, const float* w, const float* b, float* out_f32,
                               void* out_act, int precision, int64_t rows, int dim, float eps, samaudio_stream stream) {
  if (!x || !w || !b) return bad("layernorm_rows: null x / w / b");
  if (!out_f32 && !out_act) return bad("layernorm_rows: out_f32 and out_act are both null");
  if (rows <= 0) return bad("layernorm_rows: rows <= 0");
  if (dim <= 0 || dim % 4) return bad("layernorm_rows: dim % 4 (and dim > 0)");
  if (x_ld % 4) return bad("layernorm_rows: x_ld % 4");
  if (x_ld < dim) return bad("layernorm_rows: x_ld < dim");
  if (!al16(x) || !al16(w) || !al16(b) || !al16(out_f32) || !al_out(out_act, precision))
    return bad("layernorm_rows: x, w, b and out_f32 must be aligned to 16 bytes, out_act to 16 (fp32) / 8 (16-bit)");
  return hip_ret(sa::launch_layernorm_rows(x, x_ld, w, b, out_f32, out_act, precision == SAMAUDIO_BF16, rows, dim, eps,
                                           (hipStream_t)stream), "layernorm_rows");
}

int samaudio_op_layernorm_rows_split3(const float* x, int64_t x_ld, const float* w, const float* b, void* out3, int64_t rows,
                                      int dim, float eps, samaudio_stream stream) {
  if (!x || !w || !b || !out3 || rows <= 0 || dim <= 0 || dim % 8 || dim > 2048 || x_ld % 4)
    return bad("layernorm_rows_split3: null argument / dim % 8, dim <= 2048, x_ld % 4");
  if (!sa::launch_layernorm_rows_split3) {
    g_err = "layernorm_rows_split3: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  return hip_ret(sa::launch_layernorm_rows_split3(x, x_ld, w, b, out3, rows, dim, eps, (hipStream_t)stream), "layernorm_rows_split3");
}

int samaudio_op_resize_frames(const uint8_t* frames, int n, int height, int width, int out_size, int mode, float* out,
                              samaudio_stream stream) {
  if (!frames || !out || n <= 0 || height < 1 || width < 1 || out_size < 1)
    return bad("resize_frames: null argument / n, height, width, out_size < 1");
  if (mode != SAMAUDIO_RESIZE_NEAREST && mode != SAMAUDIO_RESIZE_BILINEAR && mode != SAMAUDIO_RESIZE_BICUBIC)
    return bad("resize_frames: unknown mode");
  if (!sa::launch_resize_frames) {
    g_err = "resize_frames: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  return hip_ret(sa::launch_resize_frames(frames, n, height, width, out_size, mode, out, false, 0, 0, (hipStream_t)stream),
                 "resize_frames");
}

int samaudio_op_resize_video(const uint8_t* frames, int64_t src_frames, int height, int width, const uint8_t* mask, int mask_channels,
                             const int32_t* pick, int n, int out_size, int mode, float* out, samaudio_stream stream) {
  if (!frames || !out || src_frames < 1 || src_frames > INT32_MAX || n < 1 || height < 1 || width < 1 || out_size < 1)
    return bad("resize_video: null argument / src_frames, n, height, width, out_size < 1");
  if (mask && mask_channels != 1 && mask_channels != 3) return bad("resize_video: mask_channels must be 1 or 3");
  if (mode != SAMAUDIO_RESIZE_NEAREST && mode != SAMAUDIO_RESIZE_BILINEAR && mode != SAMAUDIO_RESIZE_BICUBIC)
    return bad("resize_video: unknown mode");
  if (!pick && n != src_frames) return bad("resize_video: no pick table, but n != src_frames");
  if (!sa::launch_resize_video) {
    g_err = "resize_video: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  return hip_ret(sa::launch_resize_video(frames, (long)src_frames, height, width, mask, mask_channels, pick, n, out_size, mode, out,
                                         false, 0, 0, (hipStream_t)stream),
                 "resize_video");
}

int64_t samaudio_resample_length(int64_t samples, int step, int phases) {
  if (samples < 1 || step < 1 || phases < 1) return -1;
  const int64_t whole = samples / step, rest = samples % step;   // (phases * rest < 2^62; phases * samples may not fit)
  if (whole > (INT64_MAX >> 32)) return -1;
  return phases * whole + (phases * rest + step - 1) / step;
}

int samaudio_op_resample(const void* pcm, int fmt, int channels, int64_t samples, int64_t ch_stride, int64_t s_stride,
                         const float* taps, const int32_t* first, int phases, int step, int taps_per_phase, float* out,
                         int64_t out_capacity, samaudio_stream stream) {
  if (!pcm || !taps || !first || !out || channels < 1 || samples < 1 || step < 1 || phases < 1 || taps_per_phase < 1)
    return bad("resample: null argument / channels, samples, step, phases, taps_per_phase < 1");
  if (fmt != SAMAUDIO_PCM_S16 && fmt != SAMAUDIO_PCM_F32) return bad("resample: unknown format");
  const int64_t length = samaudio_resample_length(samples, step, phases);
  if (length < 0 || out_capacity < length) return bad("resample: out_capacity below the resampled length");
  if (!sa::launch_resample_mix) {
    g_err = "resample: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  return hip_ret(sa::launch_resample_mix(pcm, fmt == SAMAUDIO_PCM_S16, channels, samples, ch_stride, s_stride, taps, first, phases,
                                         step, taps_per_phase, out, length, out_capacity, (hipStream_t)stream),
                 "resample");
}

// ---- sound activity --------------------------------------------------------------------------------------------
// N = floor(phases (samples - 1) / step) + 1 frames at 24 kHz (audioop.ratecv's length); -1 for an argument it refuses
static int64_t activity_frames(int64_t samples, int step, int phases) {
  if (samples < 1 || step < 1 || phases < 1 || 24000 % phases) return -1;
  const int64_t whole = (samples - 1) / step, rest = (samples - 1) % step;
  if (whole > (INT64_MAX >> 32)) return -1;
  return phases * whole + phases * rest / step + 1;
}

int64_t samaudio_activity_length_ms(int64_t samples, int step, int phases) {
  const int64_t frames = activity_frames(samples, step, phases);
  if (frames < 0) return -1;
  const int64_t q = frames / 24, r = frames % 24;   // round(1000 N / 24000), ties to even
  return q + ((r > 12 || (r == 12 && (q & 1))) ? 1 : 0);
}

int64_t samaudio_activity_workspace_bytes(int rows, int64_t samples, int step, int phases) {
  const int64_t length = samaudio_activity_length_ms(samples, step, phases);
  if (rows < 1 || length < 0) return -1;
  return (int64_t)rows * (length > 0 ? length : 1) * (int64_t)sizeof(int64_t);
}

int samaudio_op_activity(const float* wav, int rows, int64_t row_stride, int64_t samples, int step, int phases,
                         const int32_t* threshold_table, const double* ref_spans, int n_ref, int metric, void* workspace,
                         int64_t workspace_bytes, float* scores, int32_t* spans, int max_spans, int32_t* span_count, int32_t* peak,
                         samaudio_stream stream) {
  if (!wav || !threshold_table || !workspace || !scores) return bad("activity: null wav / threshold_table / workspace / scores");
  if (rows < 1 || samples < 1 || step < 1 || phases < 1) return bad("activity: rows, samples, step, phases < 1");
  if (24000 % phases) return bad("activity: phases must divide 24000 (phases = 24000 / gcd(rate, 24000))");
  if (row_stride < samples) return bad("activity: row_stride below samples");
  if (metric < 0 || metric > 2) return bad("activity: metric must be 0 (iou), 1 (recall) or 2 (precision)");
  if (n_ref < 0 || (n_ref > 0 && !ref_spans)) return bad("activity: n_ref < 0, or n_ref > 0 without ref_spans");
  const int64_t frames = activity_frames(samples, step, phases);
  const int64_t length = samaudio_activity_length_ms(samples, step, phases);
  const int64_t need = samaudio_activity_workspace_bytes(rows, samples, step, phases);
  if (frames < 0 || length < 0 || length > INT32_MAX) return bad("activity: clip too long");
  if (need < 0 || workspace_bytes < need || (uintptr_t)workspace % sizeof(int64_t))
    return bad("activity: workspace below samaudio_activity_workspace_bytes, or not aligned to 8 bytes");
  if (spans && max_spans < length / 250 + 1) return bad("activity: max_spans below L / 250 + 1");
  if (!sa::launch_activity) {
    g_err = "activity: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  return hip_ret(sa::launch_activity(wav, rows, (long)row_stride, step, phases, (long)frames, (long)length, threshold_table, ref_spans,
                                     n_ref, metric, (long long*)workspace, scores, spans, max_spans, span_count, peak,
                                     (hipStream_t)stream),
                 "activity");
}

// ---- CLAP log-mel front end ------------------------------------------------------------------------------------------
int64_t samaudio_logmel_frames(int64_t max_length, int hop) {
  if (max_length < 1 || hop < 1) return -1;
  return 1 + max_length / hop;
}

int samaudio_op_logmel(const float* wav, int rows, int64_t row_stride, const int64_t* lengths, const int64_t* offsets,
                       int64_t max_length, int quantise, int fft_size, int hop, int n_mels, const float* tables, const float* bank,
                       const float* bn_scale, const float* bn_shift, float* out, samaudio_stream stream) {
  if (!wav || !lengths || !tables || !bank || !out) return bad("logmel: null wav / lengths / tables / bank / out");
  if ((bn_scale == nullptr) != (bn_shift == nullptr)) return bad("logmel: bn_scale and bn_shift go together");
  if (rows < 1 || rows > 65535 || hop < 1 || n_mels < 1) return bad("logmel: rows outside [1, 65535], hop or n_mels < 1");
  int log2n = 0;
  while ((1 << log2n) < fft_size && log2n < 12) ++log2n;
  if (fft_size < 64 || fft_size > 2048 || (1 << log2n) != fft_size) return bad("logmel: fft_size must be a power of two in [64, 2048]");
  if (max_length <= fft_size / 2 || max_length >= (1LL << 30))
    return bad("logmel: max_length must be above fft_size / 2 (the reflection) and below 2^30");
  for (int r = 0; r < rows; ++r) {
    if (lengths[r] < 1) return bad("logmel: a clip of length < 1");
    if (rows > 1 && lengths[r] > row_stride) return bad("logmel: a clip longer than row_stride");
    if (lengths[r] > max_length && offsets && (offsets[r] < 0 || offsets[r] > lengths[r] - max_length))
      return bad("logmel: a crop offset outside [0, length - max_length]");
  }
  if (!sa::launch_clap_logmel) {
    g_err = "logmel: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  const int frames = (int)samaudio_logmel_frames(max_length, hop);
  const auto offset_of = [&](int r) { return lengths[r] > max_length && offsets ? offsets[r] : (int64_t)0; };
  for (int r0 = 0; r0 < rows;) {   // consecutive rows of one length and offset share a launch
    int r1 = r0 + 1;
    while (r1 < rows && lengths[r1] == lengths[r0] && offset_of(r1) == offset_of(r0)) ++r1;
    const hipError_t e = sa::launch_clap_logmel(wav + (int64_t)r0 * row_stride, r1 - r0, (long)row_stride, (long)lengths[r0],
                                                (long)offset_of(r0), (int)max_length, quantise != 0, log2n, hop, n_mels, frames, tables,
                                                bank, bn_scale, bn_shift, out + (int64_t)r0 * frames * n_mels, (hipStream_t)stream);
    if (e != hipSuccess) return hip_ret(e, "logmel");
    r0 = r1;
  }
  return SAMAUDIO_OK;
}

int samaudio_op_window_blend(float* out, const int32_t* next_row, int rows, int frames, int overlap, int channels,
                             samaudio_stream stream) {
  if (!out || !next_row || rows < 1 || frames < 2) return bad("window_blend: null out / next_row, rows < 1 or frames < 2");
  if (overlap < 1 || overlap > frames / 2) return bad("window_blend: overlap must be in [1, frames / 2]");
  if (channels < 4 || channels % 4) return bad("window_blend: channels % 4 != 0");
  if (((uintptr_t)out & 15) || ((uintptr_t)next_row & 3)) return bad("window_blend: out must be aligned to 16 bytes, next_row to 4");
  if (!sa::launch_window_blend) {
    g_err = "window_blend: not in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  return hip_ret(sa::launch_window_blend(out, next_row, rows, frames, overlap, channels, (hipStream_t)stream), "window_blend");
}

int samaudio_op_split3(const float* x, int64_t x_ld, void* out, int64_t rows, int k, samaudio_stream stream) {
  if (!x || !out || rows <= 0 || k <= 0 || k % 8 || x_ld % 4) return bad("split3: k % 8, x_ld % 4");
  return hip_ret(sa::launch_split3(x, x_ld, out, rows, k, (hipStream_t)stream), "split3");
}

// ---- hooks of the kernels a DiT layer launches (tests/test_layer_kernels_gpu.py) ----------------------------
int samaudio_op_mod_tables(const float* const* w, const float* const* shift_tab, const float* const* scale_tab,
                           const int* shift_off, const int* scale_off, int n_norms, const float* tvec, int64_t tvec_ld,
                           int n_time, float* gs, int dim, samaudio_stream stream) {
  if (!w || !shift_tab || !scale_tab || !shift_off || !scale_off || !tvec || !gs) return bad("mod_tables: null argument");
  if (n_norms <= 0 || n_norms > sa::kMaxModNorms || n_time <= 0 || dim <= 0) return bad("mod_tables: n_norms / n_time / dim");
  sa::ModTables mt;
  for (int n = 0; n < sa::kMaxModNorms; ++n) {
    const bool on = n < n_norms;
    mt.w[n] = on ? w[n] : nullptr;
    mt.shift_tab[n] = on ? shift_tab[n] : nullptr;
    mt.scale_tab[n] = on ? scale_tab[n] : nullptr;
    mt.shift_off[n] = on ? shift_off[n] : 0;
    mt.scale_off[n] = on ? scale_off[n] : 0;
  }
  return hip_ret(sa::launch_mod_tables(mt, n_norms, tvec, tvec_ld, n_time, gs, dim, (hipStream_t)stream), "mod_tables");
}

int samaudio_op_rmsnorm_gs(const float* x, const float* gs, int64_t gs_ld, void* out, int precision, int form, int rows,
                           int dim, int rows_per_batch, float eps, samaudio_stream stream) {
  if (dim <= 0 || dim % 4 || dim > 3072) return bad("rmsnorm_gs: dim % 4, dim <= 3072");
  if (rows <= 0 || rows_per_batch <= 0 || gs_ld % 4) return bad("rmsnorm_gs: rows / rows_per_batch / gs_ld % 4");
  const bool bf16 = precision == SAMAUDIO_BF16;
  if (form == 2) {
    if (bf16) return bad("rmsnorm_gs: the split form belongs to fp32 contexts");
    return hip_ret(sa::launch_rmsnorm_gs_split3(x, gs, gs_ld, out, rows, dim, rows_per_batch, eps, (hipStream_t)stream),
                   "rmsnorm_gs_split3");
  }
  if (form != 0 && form != 1) return bad("rmsnorm_gs: form");
  if (form == 1 && !bf16) return bad("rmsnorm_gs: the alt-16 form belongs to 16-bit contexts");
  return hip_ret(sa::launch_rmsnorm_gs(x, gs, gs_ld, out, bf16, rows, dim, rows_per_batch, eps, (hipStream_t)stream, form == 1),
                 "rmsnorm_gs");
}

int samaudio_op_qkv_prep_hd(const void* qkv, const float* q_w, const float* k_w, const float* rope_cos,
                            const float* rope_sin, void* q, void* k, void* vt, int precision, int form, int batch,
                            int frames, int frames_padded, int heads, int head_dim, float eps, samaudio_stream stream) {
  if (frames_padded % 64 || frames_padded < frames || frames <= 0) return bad("qkv_prep_hd: frames_padded");
  if (head_dim != 64 && head_dim != 128) return bad("qkv_prep_hd: head_dim");
  if (form == 1) {
    if (precision != SAMAUDIO_F32 || head_dim != 128) return bad("qkv_prep_hd: the f32x form takes fp32 tensors and head_dim 128");
    return hip_ret(sa::launch_qkv_prep_f32x((const float*)qkv, q_w, k_w, rope_cos, rope_sin, (float*)q, (float*)k, (float*)vt, batch,
                                            frames, frames_padded, heads, eps, (hipStream_t)stream), "qkv_prep_f32x");
  }
  if (form != 0) return bad("qkv_prep_hd: form");
  return hip_ret(sa::launch_qkv_prep(qkv, q_w, k_w, rope_cos, rope_sin, q, k, vt, precision == SAMAUDIO_BF16, batch, frames,
                                     frames_padded, heads, eps, (hipStream_t)stream, head_dim), "qkv_prep");
}

int samaudio_op_self_attention_hd(const void* q, const void* k, const void* vt, const uint8_t* key_mask, void* out,
                                  int precision, int form, int batch, int frames, int frames_padded, int heads,
                                  int head_dim, samaudio_stream stream) {
  if (frames_padded % 64 || frames_padded < frames || frames <= 0) return bad("self_attention_hd: frames_padded");
  if (head_dim != 64 && head_dim != 128) return bad("self_attention_hd: head_dim");
  if (precision < 0 || precision > 2 || form < 0 || form > 2) return bad("self_attention_hd: precision / form");
  if (form == 1 && precision != SAMAUDIO_BF16) return bad("self_attention_hd: the alt-16 output belongs to the 16-bit kernel");
  if (form == 2 && precision != 2) return bad("self_attention_hd: the split output belongs to the compensated kernel");
  if (precision == 2)
    return hip_ret(sa::launch_self_attention_x3((const float*)q, (const float*)k, (const float*)vt, key_mask,
                                                form == 2 ? nullptr : (float*)out, batch, frames, frames_padded, heads, head_dim,
                                                (hipStream_t)stream, form == 2 ? out : nullptr), "self_attention_x3");
  return hip_ret(sa::launch_self_attention_hd(q, k, vt, key_mask, out, precision == SAMAUDIO_BF16, batch, frames, frames_padded,
                                              heads, head_dim, (hipStream_t)stream, form == 1), "self_attention_hd");
}

int samaudio_op_cross_attention_hd(const void* q, const float* q_w, void* kv, int64_t kv_ld, const float* k_w,
                                   const uint8_t* mask, void* out, int precision, int batch, int frames, int text_len,
                                   int heads, int head_dim, float eps, samaudio_stream stream) {
  if (head_dim != 64 && head_dim != 128) return bad("cross_attention_hd: head_dim");
  if (batch <= 0 || frames <= 0 || text_len <= 0 || heads <= 0 || kv_ld < 2L * heads * head_dim || kv_ld % 8)
    return bad("cross_attention_hd: shape / kv_ld");
  const bool bf16 = precision == SAMAUDIO_BF16;
  hipError_t e = sa::launch_headnorm(kv, k_w, bf16, batch * text_len, kv_ld, 0, heads, eps, (hipStream_t)stream, head_dim);
  if (e != hipSuccess) return hip_ret(e, "headnorm");
  return hip_ret(sa::launch_cross_attention(q, q_w, kv, kv_ld, mask, out, bf16, batch, frames, text_len, heads, eps,
                                            (hipStream_t)stream, head_dim), "cross_attention");
}

int samaudio_op_cross_attn_probs(const void* q, const float* q_w, const void* kv, int64_t kv_ld, const uint8_t* mask, void* p,
                                 int ldp, int batch, int frames, int text_len, int ltp, int heads, float eps,
                                 samaudio_stream stream) {
  if ((ltp != 8 && ltp != 16) || text_len <= 0 || text_len > ltp || ldp < heads * ltp || ldp % 4 || kv_ld < 2L * heads * 128 || kv_ld % 8)
    return bad("cross_attn_probs: shape");
  if (batch <= 0 || frames <= 0 || heads <= 0) return bad("cross_attn_probs: batch / frames / heads");
  return hip_ret(sa::launch_cross_attn_probs(q, q_w, kv, kv_ld, mask, p, ldp, batch, frames, text_len, ltp, heads, eps,
                                             (hipStream_t)stream), "cross_attn_probs");
}

int samaudio_op_cross_attn_probs3(const float* q, const float* q_w, const float* kv, int64_t kv_ld, const uint8_t* mask, void* p3,
                                  int kp, int batch, int frames, int text_len, int ltp, int heads, float eps,
                                  samaudio_stream stream) {
  if ((ltp != 8 && ltp != 16) || text_len <= 0 || text_len > ltp || kp < heads * ltp || kp % 8 || kv_ld < 2L * heads * 128 || kv_ld % 4)
    return bad("cross_attn_probs3: shape");
  if (batch <= 0 || frames <= 0 || heads <= 0) return bad("cross_attn_probs3: batch / frames / heads");
  return hip_ret(sa::launch_cross_attn_probs3(q, q_w, kv, kv_ld, mask, p3, kp, batch, frames, text_len, ltp, heads, eps,
                                              (hipStream_t)stream), "cross_attn_probs3");
}

int samaudio_op_cross_attn_fold3(const float* wo, const float* kv, int64_t kv_ld, void* ut3, int kp, int batch, int text_len,
                                 int ltp, int heads, samaudio_stream stream) {
  if ((ltp != 8 && ltp != 16) || text_len <= 0 || text_len > ltp || kp % 64 || kp < heads * ltp || kv_ld < 2L * heads * 128 || kv_ld % 4)
    return bad("cross_attn_fold3: shape");
  if (batch <= 0 || heads <= 0) return bad("cross_attn_fold3: batch / heads");
  return hip_ret(sa::launch_cross_attn_fold3_layers(&wo, 1, kv, kv_ld, ut3, kp, batch, text_len, ltp, heads, (hipStream_t)stream),
                 "cross_attn_fold3");
}

// ---- hooks of the kernels only the towers launch (tests/test_tower_kernels_gpu.py) --------------------------
// Each refuses what its kernel cannot do - limits that otherwise live in t5.hip, mbert.hip, clap.hip, vit.hip and peav.hip - and calls
// the launcher; no arithmetic here.  The launchers of t5_kernels.hip / vit_kernels.hip are weak (kernels.h).
namespace {
int not_built(const char* what) {
  g_err = std::string(what) + ": not in this build of the library";
  return SAMAUDIO_ERR_STATE;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int kMaxGridYZ = 65535;
}  // namespace

int samaudio_op_tower_attention(const void* qkv, const uint8_t* mask, const float* bias, void* out, int precision, int batch,
                                int tokens, int heads, int head_dim, int max_len, float scale, int window, samaudio_stream stream) {
  if (!qkv || !mask || !out) return bad("tower_attention: null qkv / mask / out");
  if (precision != SAMAUDIO_F32 && precision != SAMAUDIO_BF16) return bad("tower_attention: precision");
  if (tokens < 1 || tokens > 512) return bad("tower_attention: tokens outside [1, 512]");
  if (head_dim < 1 || head_dim > 128) return bad("tower_attention: head_dim outside [1, 128]");
  if (batch < 1 || batch > kMaxGridYZ || heads < 1 || heads > kMaxGridYZ) return bad("tower_attention: batch / heads");
  if (bias && max_len < tokens) return bad("tower_attention: a bias table of max_len < tokens");
  if (!sa::launch_t5_attention) return not_built("tower_attention");
  return hip_ret(sa::launch_t5_attention(qkv, mask, bias, out, precision == SAMAUDIO_BF16, batch, tokens, heads, head_dim, max_len,
                                         scale, window, (hipStream_t)stream), "tower_attention");
}

int samaudio_op_mbert_rope(void* qkv, const float* rope_cos, const float* rope_sin, int precision, int64_t rows, int tokens, int heads,
                           int head_dim, samaudio_stream stream) {
  if (!qkv || !rope_cos || !rope_sin) return bad("mbert_rope: null argument");
  if (precision != SAMAUDIO_F32 && precision != SAMAUDIO_BF16) return bad("mbert_rope: precision");
  if (head_dim < 2 || head_dim % 2) return bad("mbert_rope: odd head_dim");
  if (rows < 1 || rows > INT32_MAX || tokens < 1 || heads < 1) return bad("mbert_rope: rows / tokens / heads");
  if (!sa::launch_mbert_rope) return not_built("mbert_rope");
  return hip_ret(sa::launch_mbert_rope(qkv, rope_cos, rope_sin, precision == SAMAUDIO_BF16, (long)rows, tokens, heads, head_dim,
                                       (hipStream_t)stream), "mbert_rope");
}

int samaudio_op_geglu(const void* x, void* out, int precision, int64_t rows, int features, samaudio_stream stream) {
  if (!x || !out) return bad("geglu: null argument");
  if (precision != SAMAUDIO_F32 && precision != SAMAUDIO_BF16) return bad("geglu: precision");
  if (rows < 1 || features < 1) return bad("geglu: rows / features");
  if (!sa::launch_geglu) return not_built("geglu");
  return hip_ret(sa::launch_geglu(x, out, precision == SAMAUDIO_BF16, (long)rows, features, (hipStream_t)stream), "geglu");
}

int samaudio_op_rope2d_split(const void* qkv, const float* rope_cos, const float* rope_sin, void* q, void* k, void* vt, int precision,
                             int n, int tokens, int tokens_padded, int heads, int head_dim, samaudio_stream stream) {
  if (!qkv || !q || !k || !vt) return bad("rope2d_split: null argument");
  if ((rope_cos == nullptr) != (rope_sin == nullptr)) return bad("rope2d_split: rope_cos and rope_sin go together");
  if (precision != SAMAUDIO_F32 && precision != SAMAUDIO_BF16) return bad("rope2d_split: precision");
  if (head_dim != 64 && head_dim != 128) return bad("rope2d_split: head_dim");
  if (tokens < 1 || tokens_padded % 64 || tokens_padded < tokens) return bad("rope2d_split: tokens_padded");
  if (n < 1 || n > kMaxGridYZ || heads < 1 || heads > kMaxGridYZ) return bad("rope2d_split: n / heads");
  if (precision == SAMAUDIO_BF16 && !(aligned16(qkv) && aligned16(q) && aligned16(k) && aligned16(vt) && aligned16(rope_cos) &&
                                      aligned16(rope_sin)))
    return bad("rope2d_split: the 16-bit kernel moves 16 bytes per lane - every pointer must be aligned to 16 bytes");
  if (precision == SAMAUDIO_F32 && (((uintptr_t)qkv | (uintptr_t)q | (uintptr_t)k) & 7))
    return bad("rope2d_split: qkv, q and k must be aligned to 8 bytes");
  if (!sa::launch_rope2d_split) return not_built("rope2d_split");
  return hip_ret(sa::launch_rope2d_split(qkv, rope_cos, rope_sin, q, k, vt, precision == SAMAUDIO_BF16, n, tokens, tokens_padded, heads,
                                         head_dim, (hipStream_t)stream), "rope2d_split");
}

int samaudio_op_pool_attention(const float* q, const void* kv, void* out, int precision, int n, int tokens, int heads, int head_dim,
                               samaudio_stream stream) {
  if (!q || !kv || !out) return bad("pool_attention: null argument");
  if (precision != SAMAUDIO_F32 && precision != SAMAUDIO_BF16) return bad("pool_attention: precision");
  if (head_dim != 64 && head_dim != 128) return bad("pool_attention: head_dim");
  if (tokens < 1) return bad("pool_attention: tokens < 1");
  if (n < 1 || n > kMaxGridYZ || heads < 1) return bad("pool_attention: n / heads");
  if (!sa::launch_pool_attention) return not_built("pool_attention");
  return hip_ret(sa::launch_pool_attention(q, kv, out, precision == SAMAUDIO_BF16, n, tokens, heads, head_dim, (hipStream_t)stream),
                 "pool_attention");
}

int samaudio_op_l2_normalize(float* x, int rows, int dim, samaudio_stream stream) {
  if (!x || rows < 1 || dim < 1) return bad("l2_normalize: null x / rows, dim < 1");
  if (!sa::launch_l2_normalize) return not_built("l2_normalize");
  return hip_ret(sa::launch_l2_normalize(x, rows, dim, (hipStream_t)stream), "l2_normalize");
}

int samaudio_op_token_mean(const float* x, int64_t x_ld, float* out_f32, void* out_act, int precision, int n, int tokens, int dim,
                           samaudio_stream stream) {
  if (!x) return bad("token_mean: null x");
  if (!out_f32 && !out_act) return bad("token_mean: both outputs null");
  if (precision != SAMAUDIO_F32 && precision != SAMAUDIO_BF16) return bad("token_mean: precision");
  if (n < 1 || tokens < 1 || dim < 1 || x_ld < dim) return bad("token_mean: n, tokens, dim < 1 or x_ld < dim");
  if (!sa::launch_token_mean) return not_built("token_mean");
  return hip_ret(sa::launch_token_mean(x, (long)x_ld, out_f32, out_act, precision == SAMAUDIO_BF16, n, tokens, dim, (hipStream_t)stream),
                 "token_mean");
}

int samaudio_op_peav_cls_mask(float* h, const float* cls, const uint8_t* pad, uint8_t* mask_s, int batch, int frames, int dim,
                              samaudio_stream stream) {
  if (!h || !cls || !mask_s) return bad("peav_cls_mask: null h / cls / mask_s");
  if (batch < 1 || frames < 1 || dim < 4 || dim % 4) return bad("peav_cls_mask: batch, frames < 1 or dim % 4");
  if (!aligned16(h) || !aligned16(cls)) return bad("peav_cls_mask: h and cls must be aligned to 16 bytes");
  return hip_ret(sa::launch_peav_cls_mask(h, cls, pad, mask_s, batch, frames, dim, (hipStream_t)stream), "peav_cls_mask");
}

int samaudio_op_judge_pool_head(const float* hidden, const uint8_t* mask_s, const float* head_w, const float* mean, const float* std_,
                                float* out, int batch, int frames, int dim, samaudio_stream stream) {
  if (!hidden || !mask_s || !head_w || !mean || !std_ || !out) return bad("judge_pool_head: null argument");
  if (dim < 1 || dim > 4096) return bad("judge_pool_head: dim outside [1, 4096] (the pooled row lives in LDS)");
  if (batch < 1 || frames < 1) return bad("judge_pool_head: batch / frames");
  return hip_ret(sa::launch_judge_pool_head(hidden, mask_s, head_w, mean, std_, out, batch, frames, dim, (hipStream_t)stream),
                 "judge_pool_head");
}

int samaudio_op_frame_logits(const float* audio, int64_t a_bstride, int64_t a_off, const float* text, const float* scale,
                             const float* bias, float* out, int batch, int frames, int embed_dim, samaudio_stream stream) {
  if (!audio || !text || !scale || !bias || !out) return bad("frame_logits: null argument");
  if (embed_dim < 4 || embed_dim % 4) return bad("frame_logits: embed_dim % 4");
  if (a_off < 0 || a_off % 4 || a_bstride < 0 || a_bstride % 4) return bad("frame_logits: a_off % 4 / a_bstride % 4");
  if (batch < 1 || frames < 1) return bad("frame_logits: batch / frames");
  if (!aligned16(audio) || !aligned16(text)) return bad("frame_logits: audio and text must be aligned to 16 bytes");
  return hip_ret(sa::launch_frame_logits(audio, (long)a_bstride, (long)a_off, text, scale, bias, out, batch, frames, embed_dim,
                                         (hipStream_t)stream), "frame_logits");
}

// ---- hooks of the glue kernels between those (tests/test_glue_kernels_gpu.py) -------------------------------
// The same rule: argument checks, then the launcher the engine / the towers call, unchanged.  launch_ode_stage, launch_t5_embed and
// launch_clap_text_embed are weak (kernels.h); so is sa::sentinel_built, defined beside the real launch_sentinel only (the emulation's is a stub).
namespace {
bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }
bool storage(int precision) { return precision == SAMAUDIO_F32 || precision == SAMAUDIO_BF16; }
}  // namespace

int samaudio_op_time_features(const float* t, int n_time, const float* freqs, int freq_dim, const float* inv_freq, int dim, void* temb,
                              float* tsin, int precision, samaudio_stream stream) {
  if (!t || !freqs || !inv_freq || !temb || !tsin) return bad("time_features: null argument");
  if (!storage(precision)) return bad("time_features: precision");
  if (n_time < 1) return bad("time_features: n_time < 1");
  if (freq_dim < 2 || freq_dim % 2) return bad("time_features: odd freq_dim");
  if (dim < 2 || dim % 2) return bad("time_features: odd dim");
  return hip_ret(sa::launch_time_features(t, n_time, freqs, freq_dim, inv_freq, dim, temb, tsin, precision == SAMAUDIO_BF16,
                                          (hipStream_t)stream), "time_features");
}

int samaudio_op_add_rowvec(const float* x, const float* vec, int64_t vec_ld, void* out, int precision, int rows, int dim,
                           int rows_per_batch, samaudio_stream stream) {
  if (!x || !vec || !out) return bad("add_rowvec: null argument");
  if (!storage(precision)) return bad("add_rowvec: precision");
  if (rows < 1 || rows_per_batch < 1) return bad("add_rowvec: rows / rows_per_batch < 1");
  if (dim < 4 || dim % 4) return bad("add_rowvec: dim % 4");
  if (vec_ld < 0 || vec_ld % 4) return bad("add_rowvec: vec_ld % 4");
  if (!aligned16(x) || !aligned16(vec) || !aligned_to(out, precision == SAMAUDIO_BF16 ? 8 : 16))
    return bad("add_rowvec: x and vec must be aligned to 16 bytes, out to 16 (fp32) / 8 (16-bit)");
  return hip_ret(sa::launch_add_rowvec(x, vec, (long)vec_ld, out, precision == SAMAUDIO_BF16, rows, dim, rows_per_batch,
                                       (hipStream_t)stream), "add_rowvec");
}

int samaudio_op_headnorm_layers(void* kv_all, const float* w_all, int precision, int rows, int layers, int heads, int head_dim,
                                float eps, samaudio_stream stream) {
  if (!kv_all || !w_all) return bad("headnorm_layers: null argument");
  if (!storage(precision)) return bad("headnorm_layers: precision");
  if (head_dim != 64 && head_dim != 128) return bad("headnorm_layers: head_dim");
  if (rows < 1 || layers < 1 || heads < 1) return bad("headnorm_layers: rows / layers / heads < 1");
  if (!aligned_to(kv_all, precision == SAMAUDIO_BF16 ? 4 : 8)) return bad("headnorm_layers: kv_all must be aligned to 8 (fp32) / 4 (16-bit) bytes");
  return hip_ret(sa::launch_headnorm_layers(kv_all, w_all, precision == SAMAUDIO_BF16, rows, layers, heads, eps, (hipStream_t)stream,
                                            head_dim), "headnorm_layers");
}

int samaudio_op_to_act(const float* in, int64_t in_bstride, int64_t in_ld, int in_col0, void* out, int64_t out_bstride, int precision,
                       int batch, int64_t frames, int c_in, int c_out, int halo, samaudio_stream stream) {
  if (!in || !out) return bad("to_act: null argument");
  if (!storage(precision)) return bad("to_act: precision");
  if (batch < 1 || batch > kMaxGridYZ || frames < 1 || c_in < 1 || c_out < 1) return bad("to_act: batch, frames, c_in, c_out < 1");
  if (c_in > c_out) return bad("to_act: c_in > c_out");
  if (in_bstride < 0 || in_ld < 0 || in_col0 < 0 || out_bstride < 0 || halo < 0) return bad("to_act: a negative stride / offset / halo");
  return hip_ret(sa::launch_to_act(in, (long)in_bstride, (long)in_ld, in_col0, out, (long)out_bstride, precision == SAMAUDIO_BF16, batch,
                                   (long)frames, c_in, c_out, halo, (hipStream_t)stream), "to_act");
}

int samaudio_op_zero_halo(void* buf, int precision, int batch, int64_t frames, int channels, int halo, samaudio_stream stream) {
  if (!buf) return bad("zero_halo: null buf");
  if (!storage(precision)) return bad("zero_halo: precision");
  if (batch < 1 || batch > kMaxGridYZ || frames < 1 || channels < 1 || halo < 1) return bad("zero_halo: batch, frames, channels, halo < 1");
  return hip_ret(sa::launch_zero_halo(buf, precision == SAMAUDIO_BF16, batch, (long)frames, channels, halo, (hipStream_t)stream),
                 "zero_halo");
}

int samaudio_op_anchor_gather(const float* emb, const int64_t* ids, int n_ids, const int64_t* align, void* out, int precision,
                              int batch, int frames, int embed_dim, int vocab, samaudio_stream stream) {
  if (!emb || !ids || !align || !out) return bad("anchor_gather: null argument");
  if (!storage(precision)) return bad("anchor_gather: precision");
  if (n_ids < 1 || batch < 1 || frames < 1 || embed_dim < 1 || vocab < 1) return bad("anchor_gather: n_ids, batch, frames, embed_dim, vocab < 1");
  if (!aligned_to(ids, 8) || !aligned_to(align, 8)) return bad("anchor_gather: ids and align must be aligned to 8 bytes");
  return hip_ret(sa::launch_anchor_gather(emb, (const long*)ids, n_ids, (const long*)align, out, precision == SAMAUDIO_BF16, batch,
                                          frames, embed_dim, vocab, (hipStream_t)stream), "anchor_gather");
}

int samaudio_op_set_floats(float* dst, const float* host_values, int n, samaudio_stream stream) {
  if (!dst || !host_values || n < 1) return bad("set_floats: null argument or n < 1");
  return hip_ret(sa::launch_set_floats(dst, host_values, n, (hipStream_t)stream), "set_floats");
}

int samaudio_op_noise(float* out, int clips, int candidates, int frames, int channels, uint64_t seed, const int64_t* clip_ids_host,
                      samaudio_stream stream) {
  if (!out || !clip_ids_host) return bad("noise: null out / clip_ids_host");
  if (!aligned16(out)) return bad("noise: out must be aligned to 16 bytes");
  if (clips < 1 || candidates < 1 || frames < 1) return bad("noise: clips, candidates, frames < 1");
  if (channels < 4 || channels % 4) return bad("noise: channels % 4 != 0");
  if ((uint64_t)frames * (uint64_t)(channels / 4) > (1ull << 32))
    return bad("noise: frames * channels / 4 above 2^32 (the counter's first word)");
  for (int b = 0; b < clips; ++b)
    if (clip_ids_host[b] < 0) return bad("noise: a negative clip id");
  if (!sa::launch_noise_rows) {
    g_err = "noise: not available in this build of the library";
    return SAMAUDIO_ERR_STATE;
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "the launcher takes the ids as long long");
  return hip_ret(sa::launch_noise_rows(out, clips, candidates, frames, channels, (unsigned long long)seed,
                                       (const long long*)clip_ids_host, (hipStream_t)stream), "noise");
}

int samaudio_op_ode_stage(const float* y0, const float* const* k, const float* coef, int n_src, float scale, float* out, int64_t n,
                          samaudio_stream stream) {
  if (!y0 || !k || !coef || !out) return bad("ode_stage: null argument");
  if (n_src < 1 || n_src > 4) return bad("ode_stage: n_src outside [1, 4]");
  if (n < 4 || n % 4) return bad("ode_stage: n % 4");
  if (!aligned16(y0) || !aligned16(out)) return bad("ode_stage: every pointer must be aligned to 16 bytes");
  sa::OdeStageArgs a{};
  a.n_src = n_src;
  for (int j = 0; j < 4; ++j) {   // entries n_src .. 3 travel as they are: the kernel must not look at them
    if (j < n_src && !k[j]) return bad("ode_stage: null argument");
    if (j < n_src && !aligned16(k[j])) return bad("ode_stage: every pointer must be aligned to 16 bytes");
    a.k[j] = k[j];
    a.coef[j] = coef[j];
  }
  if (!sa::launch_ode_stage) return not_built("ode_stage");
  return hip_ret(sa::launch_ode_stage(y0, a, scale, out, (long)n, (hipStream_t)stream), "ode_stage");
}

// the kernels of the adaptive solve: k / coef are host arrays of kOdeMaxSrc entries, ctl the device control blocks
namespace {
static_assert(sizeof(sa::OdeRowCtl) == 64, "samaudio.h documents the control block as 16 words");
const char* ode_sources(const float* const* k, const float* coef, int n_src, sa::OdeSrcArgs& a) {
  if (!k || !coef) return "null argument";
  if (n_src < 1 || n_src > sa::kOdeMaxSrc) return "n_src outside [1, 7]";
  a = sa::OdeSrcArgs{};
  a.n_src = n_src;
  for (int j = 0; j < sa::kOdeMaxSrc; ++j) {
    if (j < n_src && (!k[j] || !aligned16(k[j]))) return "a source is null or not aligned to 16 bytes";
    a.k[j] = k[j];
    a.coef[j] = coef[j];
  }
  return nullptr;
}
}  // namespace

int samaudio_op_ode_stage_rows(const float* y, const float* const* k, const float* coef, int n_src, const void* ctl, float* out,
                               int rows, int64_t row_elems, samaudio_stream stream) {
  if (!y || !ctl || !out) return bad("ode_stage_rows: null argument");
  sa::OdeSrcArgs a;
  if (const char* why = ode_sources(k, coef, n_src, a)) return bad((std::string("ode_stage_rows: ") + why).c_str());
  if (rows < 1 || rows > kMaxGridYZ) return bad("ode_stage_rows: rows");
  if (row_elems < 4 || row_elems % 4) return bad("ode_stage_rows: row_elems % 4");
  if (!aligned16(y) || !aligned16(out) || !aligned_to(ctl, 4)) return bad("ode_stage_rows: y and out must be aligned to 16 bytes");
  for (int j = 0; j < n_src; ++j)
    if (k[j] == out) return bad("ode_stage_rows: out must not be a source");
  if (!sa::launch_ode_stage_rows) return not_built("ode_stage_rows");
  return hip_ret(sa::launch_ode_stage_rows(y, a, (const sa::OdeRowCtl*)ctl, out, rows, (long)row_elems, (hipStream_t)stream),
                 "ode_stage_rows");
}

int samaudio_op_ode_error(const float* y, const float* ynew, const float* const* k, const float* coef, int n_src, const void* ctl,
                          const uint8_t* mask, float rtol, float atol, int use_h, float* partials, int rows, int frames, int channels,
                          samaudio_stream stream) {
  if (!y || !ctl || !partials) return bad("ode_error: null argument");
  sa::OdeSrcArgs a;
  if (const char* why = ode_sources(k, coef, n_src, a)) return bad((std::string("ode_error: ") + why).c_str());
  if (rows < 1 || rows > kMaxGridYZ || frames < 1) return bad("ode_error: rows / frames");
  if (channels < 4 || channels % 4) return bad("ode_error: channels % 4");
  if (!(rtol >= 0.f) || !(atol > 0.f)) return bad("ode_error: rtol >= 0 and atol > 0");
  if (!aligned16(y) || (ynew && !aligned16(ynew)) || !aligned_to(ctl, 4) || !aligned_to(partials, 4))
    return bad("ode_error: y and ynew must be aligned to 16 bytes");
  if (!sa::launch_ode_error) return not_built("ode_error");
  return hip_ret(sa::launch_ode_error(y, ynew, a, (const sa::OdeRowCtl*)ctl, mask, rtol, atol, use_h, partials, rows, frames, channels,
                                      (hipStream_t)stream), "ode_error");
}

int samaudio_op_ode_control(void* ctl, int mode, int method, float t0, float t1, const samaudio_ode_adaptive* opt, const float* partials,
                            const float* partials_b, int chunks, const uint8_t* mask, int frames, int channels, float* times,
                            int32_t* active, int rows, samaudio_stream stream) {
  if (!ctl || !opt || !times || !active) return bad("ode_control: null argument");
  sa::OdeControlArgs a;
  if (!sa::ode_control_args(method, t0, t1, *opt, a)) return bad("ode_control: the method must be dopri5 or bosh3");
  if (mode < sa::ODE_CTL_RESET || mode > sa::ODE_CTL_STEP) return bad("ode_control: mode");
  if (rows < 1 || frames < 1 || channels < 1) return bad("ode_control: rows, frames, channels < 1");
  if (mode != sa::ODE_CTL_RESET && (!partials || chunks < 1)) return bad("ode_control: partials");
  if (mode == sa::ODE_CTL_INIT1 && !partials_b) return bad("ode_control: the initial-step rule reads two sets of partials");
  if (!aligned_to(ctl, 4) || !aligned_to(times, 4) || !aligned_to(active, 4)) return bad("ode_control: alignment");
  if (!sa::launch_ode_control) return not_built("ode_control");
  return hip_ret(sa::launch_ode_control((sa::OdeRowCtl*)ctl, mode, a, partials, partials_b, chunks, mask, frames, channels, times,
                                        (int*)active, rows, (hipStream_t)stream), "ode_control");
}

int samaudio_op_ode_control_groups(void* ctl, int mode, int method, float t0, float t1, const samaudio_ode_adaptive* opt,
                                   const float* partials, const float* partials_b, int chunks, const uint8_t* mask, int frames,
                                   int channels, float* times, int32_t* active, int rows, const int32_t* groups, int n_groups,
                                   samaudio_stream stream) {
  if (!ctl || !opt || !times || !active) return bad("ode_control_groups: null argument");
  sa::OdeControlArgs a;
  if (!sa::ode_control_args(method, t0, t1, *opt, a)) return bad("ode_control_groups: the method must be dopri5 or bosh3");
  if (mode < sa::ODE_CTL_RESET || mode > sa::ODE_CTL_STEP) return bad("ode_control_groups: mode");
  if (rows < 1 || frames < 1 || channels < 1) return bad("ode_control_groups: rows, frames, channels < 1");
  if (mode != sa::ODE_CTL_RESET && (!partials || chunks < 1)) return bad("ode_control_groups: partials");
  if (mode == sa::ODE_CTL_INIT1 && !partials_b) return bad("ode_control_groups: the initial-step rule reads two sets of partials");
  if (groups ? n_groups < 1 : n_groups != rows) return bad("ode_control_groups: n_groups (>= 1; rows when the table is null)");
  if (!aligned_to(ctl, 4) || !aligned_to(times, 4) || !aligned_to(active, 4) || !aligned_to(groups, 4))
    return bad("ode_control_groups: alignment");
  if (!sa::launch_ode_control_groups) return not_built("ode_control_groups");
  return hip_ret(sa::launch_ode_control_groups((sa::OdeRowCtl*)ctl, mode, a, partials, partials_b, chunks, mask, frames, channels, times,
                                               (int*)active, rows, groups, n_groups, (hipStream_t)stream), "ode_control_groups");
}

int samaudio_op_ode_commit(float* y, const float* ynew, float* k_first, const float* k_last, const void* ctl, int rows,
                           int64_t row_elems, samaudio_stream stream) {
  if (!y || !ynew || !k_first || !k_last || !ctl) return bad("ode_commit: null argument");
  if (rows < 1 || rows > kMaxGridYZ) return bad("ode_commit: rows");
  if (row_elems < 4 || row_elems % 4) return bad("ode_commit: row_elems % 4");
  if (!aligned16(y) || !aligned16(ynew) || !aligned16(k_first) || !aligned16(k_last) || !aligned_to(ctl, 4))
    return bad("ode_commit: every array must be aligned to 16 bytes");
  if (!sa::launch_ode_commit) return not_built("ode_commit");
  return hip_ret(sa::launch_ode_commit(y, ynew, k_first, k_last, (const sa::OdeRowCtl*)ctl, rows, (long)row_elems, (hipStream_t)stream),
                 "ode_commit");
}

int samaudio_op_repeat_rows(const uint8_t* src, uint8_t* dst, int rows, int rep, int width, samaudio_stream stream) {
  if (!src || !dst || rows < 1 || rep < 1 || width < 1) return bad("repeat_rows: null argument or rows, rep, width < 1");
  return hip_ret(sa::launch_repeat_rows_u8(src, dst, rows, rep, width, (hipStream_t)stream), "repeat_rows");
}

int samaudio_op_repeat_items(const float* src, float* dst, int items, int rep, int64_t elems, samaudio_stream stream) {
  if (!src || !dst || items < 1 || rep < 1) return bad("repeat_items: null argument or items, rep < 1");
  if (elems < 4 || elems % 4) return bad("repeat_items: elems % 4");
  if (!aligned16(src) || !aligned16(dst)) return bad("repeat_items: src and dst must be aligned to 16 bytes");
  return hip_ret(sa::launch_repeat_items_f32(src, dst, items, rep, (long)elems, (hipStream_t)stream), "repeat_items");
}

int samaudio_op_embed_rows(const int64_t* ids, const float* table, float* out, int64_t rows, int dim, int vocab,
                           samaudio_stream stream) {
  if (!ids || !table || !out) return bad("embed_rows: null argument");
  if (rows < 1 || rows > INT32_MAX || vocab < 1) return bad("embed_rows: rows / vocab < 1");
  if (dim < 4 || dim % 4) return bad("embed_rows: dim % 4");
  if (!aligned16(table) || !aligned16(out) || !aligned_to(ids, 8)) return bad("embed_rows: table and out must be aligned to 16 bytes, ids to 8");
  if (!sa::launch_t5_embed) return not_built("embed_rows");
  return hip_ret(sa::launch_t5_embed((const long long*)ids, table, out, (long)rows, dim, vocab, (hipStream_t)stream), "embed_rows");
}

int samaudio_op_clap_text_embed(const int64_t* ids, const float* word, const float* pos, const float* type, float* out, int rows,
                                int tokens, int dim, int vocab, int pad_id, int max_positions, samaudio_stream stream) {
  if (!ids || !word || !pos || !type || !out) return bad("clap_text_embed: null argument");
  if (rows < 1 || tokens < 1 || dim < 1 || vocab < 1 || pad_id < 0) return bad("clap_text_embed: rows, tokens, dim, vocab < 1 or pad_id < 0");
  if (tokens > 1024) return bad("clap_text_embed: tokens > 1024 (the position ids of a row live in LDS)");
  if ((int64_t)pad_id + tokens + 1 > max_positions)
    return bad("clap_text_embed: the position table has fewer than pad_id + tokens + 1 rows");
  if (!aligned_to(ids, 8)) return bad("clap_text_embed: ids must be aligned to 8 bytes");
  if (!sa::launch_clap_text_embed) return not_built("clap_text_embed");
  return hip_ret(sa::launch_clap_text_embed((const long long*)ids, word, pos, type, out, rows, tokens, dim, vocab, pad_id,
                                            (hipStream_t)stream), "clap_text_embed");
}

int samaudio_op_sentinel(const void* x, int format, int64_t rows, int cols, int64_t ld, float* scratch, float* slot,
                         samaudio_stream stream) {
  if (!x || !scratch || !slot) return bad("sentinel: null argument");
  if (format < 0 || format > 2) return bad("sentinel: format outside 0..2");
  if (rows < 1 || cols < 1) return bad("sentinel: rows / cols < 1");
  if (ld < cols) return bad("sentinel: ld < cols");
  if (!aligned_to(x, format == 0 ? 4 : 2)) return bad("sentinel: x is not aligned to its element size");
  if (!sa::sentinel_built) return not_built("sentinel");
  return hip_ret(sa::launch_sentinel(x, format, (long)rows, cols, (long)ld, scratch, slot, (hipStream_t)stream), "sentinel");
}

int samaudio_op_hash_items(const uint32_t* x, int64_t words, int items, uint64_t* out, samaudio_stream stream) {
  if (!x || !out || words < 1 || items < 1) return bad("hash_items: null argument or words, items < 1");
  return hip_ret(sa::launch_hash_items((const unsigned*)x, (size_t)words, items, (unsigned long long*)out, (hipStream_t)stream),
                 "hash_items");
}

// ---- Judge reranker ----------------------------------------------------------------------------------
int samaudio_judge_create(const samaudio_judge_config* cfg, samaudio_judge** out) {
  if (!cfg || !out) return bad("samaudio_judge_create: null argument");
  if (cfg->precision != SAMAUDIO_F32 && cfg->precision != SAMAUDIO_BF16) return bad("samaudio_judge_create: precision");
  samaudio_judge* j = new samaudio_judge;
  j->judge = new sa::Judge(*cfg);
  *out = j;
  return SAMAUDIO_OK;
}

void samaudio_judge_destroy(samaudio_judge* j) {
  if (!j) return;
  delete j->judge;
  delete j;
}

int samaudio_judge_set_tensor(samaudio_judge* j, const char* name, const void* data, int dtype, int ndim,
                              const int64_t* shape) {
  return SA_ENTRY(j, "null judge", j->judge->set_tensor(name, data, dtype, ndim, shape));
}

int samaudio_judge_set_option(samaudio_judge* j, int option, int value) {
  return SA_ENTRY(j, "null judge", j->judge->set_option(option, value));
}

int samaudio_judge_finalize(samaudio_judge* j) {
  return SA_ENTRY(j, "null judge", j->judge->finalize());
}

size_t samaudio_judge_workspace_bytes(samaudio_judge* j, int inputs, int candidates, int frames) {
  if (!j) return 0;
  return j->judge->workspace_bytes(inputs, candidates, frames);
}

int samaudio_judge_set_workspace(samaudio_judge* j, void* workspace, size_t bytes) {
  return SA_ENTRY(j, "null judge", j->judge->set_workspace(workspace, bytes));
}

int samaudio_judge_score(samaudio_judge* j, const float* input_latent, const float* separated_latent, int inputs,
                         int candidates, int frames, const float* text_pooled, const uint8_t* pad_mask, float* scores,
                         samaudio_stream stream) {
  return SA_ENTRY(j, "null judge",
                  j->judge->score(input_latent, separated_latent, inputs, candidates, frames, text_pooled, pad_mask, scores,
                      (hipStream_t)stream));
}

int samaudio_judge_encode(samaudio_judge* j, int which, const float* x, const uint8_t* pad_mask, int rows, int frames,
                          float* hidden, samaudio_stream stream) {
  return SA_ENTRY(j, "null judge", j->judge->encode(which, x, pad_mask, rows, frames, hidden, (hipStream_t)stream));
}

// ---- PE-A-Frame span predictor -------------------------------------------------------------------------
int samaudio_frame_create(const samaudio_frame_config* cfg, samaudio_frame** out) {
  if (!cfg || !out) return bad("samaudio_frame_create: null argument");
  if (cfg->precision != SAMAUDIO_F32 && cfg->precision != SAMAUDIO_BF16) return bad("samaudio_frame_create: precision");
  samaudio_frame* f = new samaudio_frame;
  f->frame = new sa::FramePredictor(*cfg);
  *out = f;
  return SAMAUDIO_OK;
}

void samaudio_frame_destroy(samaudio_frame* f) {
  if (!f) return;
  delete f->frame;
  delete f;
}

int samaudio_frame_set_tensor(samaudio_frame* f, const char* name, const void* data, int dtype, int ndim,
                              const int64_t* shape) {
  return SA_ENTRY(f, "null frame predictor", f->frame->set_tensor(name, data, dtype, ndim, shape));
}

int samaudio_frame_set_option(samaudio_frame* f, int option, int value) {
  return SA_ENTRY(f, "null frame predictor", f->frame->set_option(option, value));
}

int samaudio_frame_finalize(samaudio_frame* f) {
  return SA_ENTRY(f, "null frame predictor", f->frame->finalize());
}

size_t samaudio_frame_workspace_bytes(samaudio_frame* f, int rows, int frames) {
  if (!f) return 0;
  return f->frame->workspace_bytes(rows, frames);
}

int samaudio_frame_set_workspace(samaudio_frame* f, void* workspace, size_t bytes) {
  return SA_ENTRY(f, "null frame predictor", f->frame->set_workspace(workspace, bytes));
}

int samaudio_frame_logits(samaudio_frame* f, const float* codec_features, const float* text_pooled,
                          const uint8_t* pad_mask, int rows, int frames, float* logits, samaudio_stream stream) {
  return SA_ENTRY(f, "null frame predictor",
                  f->frame->logits(codec_features, text_pooled, pad_mask, rows, frames, logits, (hipStream_t)stream));
}

}  // extern "C"
