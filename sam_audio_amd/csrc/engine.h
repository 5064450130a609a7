// Host-side orchestration of the separate() hot path: owns no device memory, sequences the kernels.
#pragma once
#include "host.h"

namespace sa {

constexpr int HALO = 40;  // zero rows either side of codec activations (>= 4 * max dilation 9)

// the controller arguments of an adaptive method (its nodes and estimator order, the caller's options); false: not an adaptive method
bool ode_control_args(int method, float t0, float t1, const samaudio_ode_adaptive& opt, OdeControlArgs& out);

class Engine {
 public:
  explicit Engine(const samaudio_config& c);
  Status set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape);
  Status finalize(int what);
  Status set_option(int option, int value);
  Status check_f32_weights(int classes) const;   // every "<name>.f32" operand copy the classes read is registered
  size_t workspace_bytes(int rows, int frames, int text_len, int codec_items, int64_t samples);
  Status set_workspace(void* p, size_t bytes);

  // `candidates` > 1: every conditioning tensor holds rows / candidates clips and serves `candidates` consecutive rows each
  // (reference model.py:193-203, sample-major); `latent_feats`: feats is the codec latent z [.., frames, latent_channels / 2] and the
  // audio features are (z | z) (model.py:182-184) - read twice through a zero tap stride, never materialised
  Status prepare(int rows, int frames, int text_len, const float* feats, const float* text, const uint8_t* text_mask,
                 const float* video, const int64_t* anchor_ids, int n_ids, const int64_t* anchor_alignment,
                 const uint8_t* pad_mask, hipStream_t st, int candidates = 1, bool latent_feats = false);
  Status forward(const float* noisy, const float* time, int n_time, float* out, hipStream_t st);
  Status ode_solve(float* state, int method, const float* grid_host, int n_grid, hipStream_t st);
  // dopri5 / bosh3 with per-row step control; synchronises `st`; stats: host, one entry per row
  Status ode_solve_adaptive(float* state, int method, float t0, float t1, const samaudio_ode_adaptive* opt,
                            samaudio_ode_row_stats* stats, hipStream_t st);
  // stage buffers of the Runge-Kutta methods (samaudio_set_ode_stages): borrowed, apart from the workspace
  struct RkTableau;   // engine.hip: rk4 / heun3
  struct AdaptiveTableau;   // engine.hip: dopri5 / bosh3
  struct AdaptiveBufs;
  size_t ode_stage_bytes(int method, int rows, int frames) const;
  Status set_ode_stages(void* p, size_t bytes);
  // windowed solve (samaudio_set_windows): while a successor table is set, every field evaluation ends with window_blend_kernel on its
  // output.  next_row: device i32 [rows], borrowed; null switches windows off, and so does every prepare
  Status set_windows(const int32_t* next_row, int rows, int overlap);
  // step control per clip for an adaptive solve over windows (samaudio_set_window_groups): groups [n_groups, 3]
  // device i32 (first row, window count, row stride) and the ownership mask [rows, frames] u8, both borrowed; only while a successor
  // table is set; null clears, and so do set_windows and every prepare
  Status set_window_groups(const int32_t* groups, int n_groups, const uint8_t* owner_mask);
  Status codec_encode(const float* wav, int items, int64_t samples, float* latent, hipStream_t st);
  // `pairs`: latent is the ODE state [items / 2, frames, 2 * codec_dim] - item 2b = the first codec_dim channels of row b (target),
  // 2b + 1 the second (residual): reference model.py:291-295 without the transposed copy
  Status codec_decode(const float* latent, int items, int frames, float* wav, hipStream_t st, bool pairs = false);
  // The same in time tiles of `tile_frames` latent frames: tile k is one pass over its frames plus
  // codec_halo_frames on each side where the clip has them, of which only the tile's own rows are written.  The scratch is sized by
  // the longest segment (codec_tile_samples), not by the clip; a tile that covers the clip is the untiled call.
  Status codec_encode_tiled(const float* wav, int items, int64_t samples, int tile_frames, float* latent, hipStream_t st);
  Status codec_decode_tiled(const float* latent, int items, int frames, int tile_frames, float* wav, hipStream_t st, bool pairs = false);
  int codec_halo_frames(bool decode) const;   // the direction's reach in whole latent frames, from the layers it launches
  int64_t codec_tile_samples(int frames, int tile_frames, bool decode) const;   // the longest segment in samples; < 0: bad argument

  // Per-kernel timing with HIP events on the launch stream (bench.py's roofline leg): between begin and end
  // every GEMM launch is bracketed by an event pair; end synchronises and folds them per tile variant.
  // name = "<class>/<kernel>": class dit | codec | prep (conditioning hoisted out of the ODE); GEMM launches carry their
  // algorithmic flops AND bytes (operands + outputs + residual, each counted once), the streaming kernels their bytes.
  struct KernelStat {
    std::string name;
    long launches = 0;
    double flops = 0, bytes = 0, ms = 0;
  };
  Status sentinel_read(float* absmax, double* nonfinite, hipStream_t st);   // SAMAUDIO_OPT_SENTINEL
  Status profile_begin();
  Status profile_end(std::vector<KernelStat>& out);
  ~Engine();

 private:
  // one field evaluation; out = res + alpha * v(noisy, t) (res may be null)
  Status eval_field(const float* noisy, const float* time, int n_time, float* out, const float* res, float alpha,
                    hipStream_t st);
  Status plan_dit(Bump& b, int rows, int frames, int text_len, bool assign);
  // the folded cross-attention for a text memory of Lt tokens, decided once (plan_dit sizes by it, prepare sets it up): tokens per head
  // slot, padded K, the 16-bit fold, the fold on compensated operands, one operand slice per layer
  struct FoldPlan { int ltp, kp; bool fold16, fold3, all_layers; };
  FoldPlan fold_plan(int Lt) const;
  // The DAC-VAE workspace, described once: carves every buffer a pass over `n` waveforms uses into `out` (null: sizing only) and returns
  // the bytes the linear model allots to n items (engine.hip kCodecFixed); codec_bytes and codec_chunk size by it, a pass checks b.fits()
  struct CodecBufs;
  size_t plan_codec(Bump& b, bool decode, int n, int64_t samples, CodecBufs* out) const;
  size_t codec_per_item(int64_t samples) const;   // the larger direction's plan_codec of one item
  size_t codec_bytes(int items, int64_t samples) const;
  int codec_chunk(int items, int64_t samples, bool pairs) const;   // items per pass in this workspace (whole pairs); 0: not even one
  Status codec_carve(bool decode, int n, int64_t samples, CodecBufs& cb);   // one pass's buffers out of the workspace
  // One pass: frames [t0, t1) of clips of T frames run through every layer, rows [keep0, keep1) of the result are written (the whole
  // pass: {0, T, 0, T, T}).  encode_pass / decode_pass hold the launches of both the untiled and the tiled calls
  struct CodecSeg { long t0, t1, keep0, keep1, T; };
  static CodecSeg codec_tile(long T, long L, long h, long k);
  Status encode_pass(const float* wav, int i0, int n, const CodecSeg& g, float* latent, hipStream_t st);
  Status decode_pass(const float* latent, int i0, int n, const CodecSeg& g, float* wav, hipStream_t st, bool pairs);
  // The kind of a GEMM launch.  F32: exact fp32 inside a 16-bit context (SAMAUDIO_OPT_F32_CLASSES - the caller hands fp32 A / W / out_act
  // pointers).  X3: a SAMAUDIO_OPT_X3_CLASSES launch inside an fp32 context (16-bit A / W over K' = 3K, fp32 outputs; linear builds it),
  // both operands split over the whole K (A rows [lo | hi | hi], W rows [W_hi | W_lo | W_hi]: the launch may share operand tiles,
  // common.h GEMM_FLAG_X3_SHARE).  X3Block: the same with K' split per input block (the convolutions of gemm_codec_x3 / the patcher:
  // [block][3 Cin]) - a plain walk over K' only
  enum class GemmKind { Native, F32, X3, X3Block };
  static GemmKind f32_if(bool f) { return f ? GemmKind::F32 : GemmKind::Native; }
  enum class Phase { Prep, Dit, Codec } phase_ = Phase::Dit;   // the profile label; Codec: launches run under the codec's kernel symbols
  const char* phase_name() const { return phase_ == Phase::Prep ? "prep" : phase_ == Phase::Dit ? "dit" : "codec"; }
  // gemm = launch_params + launch + the sentinel scan of the 16-bit output.  cls: SAMAUDIO_CLS_* bit; alg_flops < 0: 2*M*N*K*nbatch
  // (exact unless K carries zero padding, then the caller passes the true count).  The codec's convolutions go through codec_gemm.
  Status gemm(const GemmParams& p, hipStream_t st, double alg_flops, int cls, GemmKind kind = GemmKind::Native);
  GemmParams launch_params(const GemmParams& p_in, int cls, GemmKind kind) const;   // the tag / flags p_in launches with
  Status launch(GemmParams p, hipStream_t st, double alg_flops, int cls, GemmKind kind);   // one launch, profiled
  Status scan_out(const GemmParams& p, int cls, GemmKind kind, hipStream_t st);
  // One GEMM of class `cls` on the weight `w`: gemm() on w.w, or - SAMAUDIO_OPT_X3_CLASSES switched on for the class - ONE 16-bit GEMM
  // over K' = 3K on w.w3 and the split operand [lo | hi | hi] of A.  `p` = the context's plain launch (fp32 A rows, fp32-typed
  // outputs in an fp32 context).  `presplit`: A already split; otherwise split here into x3a, or into x3u when `ffn_wide` (w2's F-wide
  // operand)
  Status linear(GemmParams p, const LinW& w, int cls, hipStream_t st, const void* presplit = nullptr, bool ffn_wide = false);
  bool x3(int cls) const { return !bf16_ && (x3_classes_ & cls) != 0; }
  // A convolution of the DAC-VAE.  SAMAUDIO_OPT_X3_CLASSES bit CODEC: one with >= 256 output channels whose weight has a registered
  // "<name>.x3" twin ([N, K / Cin, 3 Cin]: every Cin-block of a weight row as [W_hi | W_lo | W_hi]) runs through gemm_codec_x3 - the fp32
  // activation buffer is split row by row into a scratch operand, the launch runs on the 8-phase 16-bit kernels over K' = 3K and an
  // elementwise kernel applies the activation to the raw fp32 result.  Everything else of the codec multiplies on operands split in
  // registers (GEMM_FLAG_X3_FLY), on the weight's "<name>.fly" twin where there is one (GEMM_FLAG_W_FLY16).
  Status codec_gemm(const GemmParams& p, hipStream_t st, double alg_flops = -1.0);
  struct X3CodecW { const void* w; int cin; };
  std::map<const void*, X3CodecW> x3_codec_;
  std::map<const void*, const void*> fly_codec_;   // fp32 codec weight -> its "<name>.fly" twin
  void* x3_codec_scratch_ = nullptr;               // the running pass's split scratch (plan_codec)
  size_t x3_codec_scratch_bytes_ = 0;
  const X3CodecW* codec_x3_twin(const GemmParams& p) const;   // the twin `p` can run on, or null
  Status gemm_codec_x3(const GemmParams& p, const X3CodecW& w, hipStream_t st, double alg_flops);
  Status check_x3_weights(int classes) const;
  bool f32c(int cls) const { return bf16_ && (f32_classes_ & cls) != 0; }
  bool alt16(int cls) const { return bf16_ && (alt_classes_ & cls) != 0; }   // SAMAUDIO_OPT_ALT16_CLASSES (mixed mode)
  const void* opt(const std::string& name, std::vector<int64_t> shape) const;  // optional fp32 tensor, null if absent / mis-shaped
  struct ProfRec {
    std::string key;
    double flops, bytes;
    hipEvent_t e0, e1;
  };
  // non-GEMM launch, event-bracketed while profiling
  template <class F>
  Status op(const char* name, double alg_bytes, double alg_flops, hipStream_t st, F&& launch);
  Status res_unit(GemmParams p, GemmParams q, void*& cur, void*& alt, double flops7, double flops1, hipStream_t st);
  struct SBuf;
  struct StageW;   // the three residual units of one codec stage on `sb`; `next_alpha`: the Snake after the last unit
  Status res_units(const StageW& sw, SBuf& sb, int n, const float* next_alpha, hipStream_t st);
  void* hash_ = nullptr;   // SAMAUDIO_TRACE_HASH recorder (engine.hip HashTrace; debugging aid)
  bool prof_on_ = false;
  std::vector<ProfRec> prof_;
  std::vector<hipEvent_t> ev_pool_;
  size_t ev_used_ = 0;
  Status prof_event(hipEvent_t* e);

  samaudio_config cfg_;
  bool bf16_;
  bool tail_split_ = true;  // SAMAUDIO_OPT_TAIL_SPLIT
  int f32_classes_ = 0;     // SAMAUDIO_OPT_F32_CLASSES (16-bit contexts)
  int alt_classes_ = 0;     // SAMAUDIO_OPT_ALT16_CLASSES (16-bit contexts)
  int prefetch_rows_ = 0;   // SAMAUDIO_OPT_PREFETCH_ROWS (16-bit contexts)
  int x3_classes_ = 0;      // SAMAUDIO_OPT_X3_CLASSES (fp32 contexts)
  Status solve_launches(float* y, int method, const float* grid, int n_grid, hipStream_t st);   // the launches of one solve
  Status solve_rk(float* y, const RkTableau& tab, const float* grid, int n_grid, hipStream_t st);   // ... of rk4 / heun3
  AdaptiveBufs adaptive_carve(const AdaptiveTableau& tab, int rows, int frames) const;   // the stage buffer of an adaptive solve
  float* stages_ = nullptr;   // samaudio_set_ode_stages
  size_t stages_bytes_ = 0;
  const int32_t* win_next_ = nullptr;   // samaudio_set_windows: the successor table of the prepared rows (null: no windows)
  int win_overlap_ = 0;
  const int32_t* win_groups_ = nullptr;   // samaudio_set_window_groups: the rows that share one step control (null: per row)
  const uint8_t* win_owner_ = nullptr;    // ... and the frames each row contributes to its group's norms
  int win_n_groups_ = 0;
  bool sentinel_on_ = false;   // SAMAUDIO_OPT_SENTINEL
  float* sentinel_dev_ = nullptr;   // [SAMAUDIO_SENTINEL_SLOTS][2] slots + [kSentinelPartials][2] partials (debug_device_alloc)
  // fold the scan of a tensor into `slot` (no-op unless the sentinel is on); fmt as launch_sentinel
  Status sentinel(int slot, const void* x, int fmt, long rows, int cols, long ld, hipStream_t st);
  int quant_classes_ = 0, quant_fmt_ = 0;  // SAMAUDIO_OPT_QUANT_CLASSES / _FORMAT (fp32 contexts)
  size_t esz_;  // bytes per activation / GEMM-operand element
  int at_dtype_;
  Registry reg_;
  bool dit_ready_ = false, codec_ready_ = false, enc_ready_ = false, prepared_ = false;
  char* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  int rows_ = 0, frames_ = 0, text_len_ = 0, frames_pad_ = 0;
  bool fold3_ = false;   // the fold runs on compensated operands (x3 context, class CWO)
  int fold_ltp_ = 0, fold_kp_ = 0;  // folded cross-attention: tokens per head slot (8 | 16; 0 = not folded), padded K
  bool has_anchor_ = false;

  // resolved weights (pointers into caller memory)
  struct LayerW {
    const float *attn_norm, *ffn_norm, *mod_table, *q_norm, *k_norm, *c_q_norm;
    LinW wqkv, wo, c_wq, c_wo, w13, w2;   // (all but c_wo may be registered K-tile-major in a 16-bit context: samaudio.h)
  };
  // a big-five weight: [N, K] row-major or (16-bit contexts) [K/64, N, 64] K-tile-major
  Status need_w5(const std::string& name, int N, int K, LinW& w) const;
  std::vector<LayerW> layers_;
  struct {
    const float *final_table, *final_norm, *gn1_w, *gn1_b, *gn2_w, *gn2_b, *pb1, *pb2, *tb_b, *t_freqs, *mem_inv_freq,
        *rope_cos, *rope_sin, *proj_b, *mem_b, *vid_b, *vid_ln_w, *vid_ln_b, *vid_gate, *anc_emb, *c_k_norm_all;
    const void *w_out, *y_w13, *y_w2, *t_w13, *t_w2, *tb_w, *proj_wy, *proj_wf, *mem_w, *vid_w, *anc_w;
    LinW pw1, pw2, c_wkv_all;   // (x3 twins: classes PATCH - "patch<n>.w.x3", per tap [W_hi | W_lo | W_hi] - and CKV)
  } g_{};
  struct {  // optional fp32 copies ("<name>.f32") of the weights of the SAMAUDIO_CLS_F32_CAPABLE classes
    const float *w_out, *t_w13, *t_w2, *tb_w, *proj_wy, *proj_wf, *mem_w, *vid_w, *anc_w, *y_w13, *y_w2;
  } g32_;
  struct ResUnitW {
    const float *a1, *b1, *a2, *b2;
    const void *w1, *w2;
    int k1pad, k2pad;
  };
  struct StageW {
    ResUnitW r[3];
    const float *a, *b;   // snake before the resampling conv, its bias
    const void* w;        // down conv [2C, 2s*C] (encoder)  /  up conv [s*Cout, 2*Cin] (decoder)
  };
  struct {
    const void *in_w, *out_w, *proj_w;
    const float *in_b, *out_a, *out_b, *proj_b;
    int out_kpad;
    StageW s[4];
  } enc_, dec_;

  // DiT workspace (assigned by plan_dit)
  struct {
    float *ymid, *aligned, *cond, *h, *hp1, *text_proj, *t_emb, *t0, *modgs, *tsin, *vtmp, *times;
    void *ybf, *xn, *qkv, *Q, *K, *Vt, *attn, *hbf, *qc, *ca, *u, *gnbuf, *mem, *yu, *yemb, *kvc, *temb, *tu, *tsilu,
        *feats, *text, *video, *anch, *probs, *ut, *x3a, *x3u, *x3p, *ut3;
    float *temb32, *tu32, *tsilu32, *xn32, *prep32, *mem32, *yu32, *yemb32;  // fp32 operands of the f32 classes (16-bit contexts)
    unsigned char *pad_mask, *text_mask;
    double* gn_part;
    size_t x3a_bytes, x3u_bytes;   // capacities of x3a / x3u (linear refuses a split that would not fit)
  } d_;
};

}  // namespace sa
