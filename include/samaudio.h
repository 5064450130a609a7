/* libsamaudio_hip.so - C ABI of the MI355X-native SAMAudio.separate() hot path.
 *
 * The reference (facebookresearch/sam-audio) is pure Python and has no FFI / operator interface; its
 * boundary is the Python class API of `sam_audio` (sam_audio/__init__.py:3-4).  This header is the
 * boundary a maintainer would bind with ctypes: plain pointers, sizes and a
 * hipStream_t - no torch types.  Each entry point cites the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - the library never allocates or frees device memory: weights are borrowed (they must outlive the
 *     context), scratch comes from one caller-provided workspace;
 *   - every call is asynchronous on `stream` (pass the caller's current HIP stream);
 *   - return value: 0 = ok, negative = error, message via samaudio_last_error();
 *   - one context per (process, GPU, stream); not thread-safe.
 */
#ifndef SAMAUDIO_H_
#define SAMAUDIO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct samaudio_ctx samaudio_ctx;
typedef void* samaudio_stream; /* hipStream_t */

enum { SAMAUDIO_F32 = 0, SAMAUDIO_BF16 = 1 };           /* compute precision == dtype of GEMM operands */
enum { SAMAUDIO_DT_F32 = 0, SAMAUDIO_DT_BF16 = 1, SAMAUDIO_DT_I64 = 2, SAMAUDIO_DT_U8 = 3 };
/* ODE methods of samaudio_ode_solve, torchdiffeq's fixed-grid solvers.  EULER and MIDPOINT fold each
 * step into the output GEMM's epilogue; RK4 (torchdiffeq's "rk4": the 3/8-rule variant, 4 evaluations per step, the last at the grid
 * point t1) and HEUN3 (Heun's third-order method, 3 evaluations) write every stage's field into a stage buffer of their own
 * (samaudio_set_ode_stages) and combine them in ode_stage_kernel.  DOPRI5 and BOSH3 are the adaptive embedded pairs of
 * samaudio_ode_solve_adaptive (below); samaudio_ode_solve answers them with SAMAUDIO_ERR_ARG. */
enum { SAMAUDIO_ODE_EULER = 0, SAMAUDIO_ODE_MIDPOINT = 1, SAMAUDIO_ODE_RK4 = 2, SAMAUDIO_ODE_HEUN3 = 3, SAMAUDIO_ODE_DOPRI5 = 4,
       SAMAUDIO_ODE_BOSH3 = 5 };

enum {
  SAMAUDIO_OK = 0,
  SAMAUDIO_ERR_ARG = -1,      /* bad argument / shape mismatch      (reference: AssertionError) */
  SAMAUDIO_ERR_WEIGHT = -2,   /* missing / mis-shaped weight tensor (reference: RuntimeError, model.py:356-359) */
  SAMAUDIO_ERR_WORKSPACE = -3,/* workspace missing or too small */
  SAMAUDIO_ERR_HIP = -4,      /* HIP runtime error */
  SAMAUDIO_ERR_STATE = -5     /* call order violated (e.g. solve before prepare) */
};

/* Hyper-parameters: reference sam_audio/model/config.py:86-135 (TransformerConfig), :204-231 (SAMAudioConfig),
 * :10-41 (DACVAEConfig). */
typedef struct {
  int32_t precision;        /* SAMAUDIO_F32 | SAMAUDIO_BF16 */
  int32_t dim, n_heads, n_layers, ffn_hidden;
  int32_t latent_channels;  /* 2 * codebook_dim = 256: ODE state width and DiT out_channels */
  int32_t text_dim;         /* 768  */
  int32_t video_dim;        /* 1024 */
  int32_t freq_dim;         /* 256  */
  int32_t anchor_dim;       /* 128  */
  int32_t anchor_vocab;     /* num_anchors + 1 = 4 */
  int32_t max_positions;    /* RoPE table rows */
  float norm_eps;
  /* DAC-VAE */
  int32_t codec_dim;        /* 128  */
  int32_t codec_latent;     /* 1024 */
  int32_t enc_dim;          /* 64   */
  int32_t dec_dim;          /* 1536 */
  int32_t enc_rates[4];     /* 2,8,10,12 */
  int32_t dec_rates[4];     /* 12,10,8,2 */
} samaudio_config;

const char* samaudio_last_error(void);
const char* samaudio_version(void);

int samaudio_create(const samaudio_config* cfg, samaudio_ctx** out);
void samaudio_destroy(samaudio_ctx* ctx);

/* Register one (re-laid-out) weight tensor by engine name; the pointer is borrowed.  The Python loader
 * (sam_audio_amd/weights.py) documents the mapping from the reference state_dict keys
 * (transformer.layers.{i}.attention.wq.weight, ...) to engine names. */
int samaudio_set_tensor(samaudio_ctx* ctx, const char* name, const void* data, int dtype, int ndim,
                        const int64_t* shape);
/* Check that the DiT (what=0), codec (what=1) or codec-encoder-only (what=2: the Judge's DACVAEEncoder,
 * reference codec.py:42-78) weight set is complete and shaped for the config. */
int samaudio_finalize(samaudio_ctx* ctx, int what);

/* Scratch.  `codec_items`: waveforms processed per codec pass (0 = no codec use), `samples`: padded
 * samples per waveform.  Besides the activations of one evaluation the DiT part holds, in 16-bit contexts with text_len <= 16 and
 * 128-wide heads, the folded cross-attention operands of ALL layers (rows * dim * pad64(heads * (8 | 16)) * n_layers 16-bit
 * elements: 0.76 GB for 32 rows at the large stand-in dims, zeroed once per samaudio_prepare), and in fp32 contexts with
 * SAMAUDIO_OPT_X3_CLASSES the split activation operands (rows * (frames + 2) * 3 * dim and rows * frames * 3 * ffn_hidden 16-bit
 * elements).  Query it AFTER setting the options that change the plan (SAMAUDIO_OPT_X3_CLASSES). */
size_t samaudio_workspace_bytes(samaudio_ctx* ctx, int rows, int frames, int text_len, int codec_items,
                                int64_t samples);
int samaudio_set_workspace(samaudio_ctx* ctx, void* workspace, size_t bytes);

/* Execution options of a context (no reference counterpart: scheduling only, results are bitwise unaffected).
 *   SAMAUDIO_OPT_TAIL_SPLIT (default 1): a GEMM whose last round of 256x256 tiles would leave most CUs idle is issued as
 *   two kernels (whole rounds + a 128x128-tile tail).  Set to 0 for contexts that share the GPU with another context's
 *   stream (SAMAudio(streams=2)): there the other stream's workgroups fill the idle CUs and the extra launches cost 2 %. */
#define SAMAUDIO_OPT_TAIL_SPLIT 1
/* Precision of single GEMM classes (the reference computes everything in fp32: README.md:48, no autocast anywhere).
 *   SAMAUDIO_OPT_F32_CLASSES (16-bit contexts; value = mask of SAMAUDIO_CLS_* bits, default 0): the named classes run on
 *   exact-fp32 operands (v_mfma_f32_16x16x4f32) inside an otherwise 16-bit context.  Needs the class's weights registered
 *   a second time in fp32 under "<name>.f32" (samaudio_set_tensor) - checked by samaudio_finalize(ctx, 0) and, on a finalized
 *   context, by samaudio_set_option itself (SAMAUDIO_ERR_WEIGHT names the missing copy); only the classes in SAMAUDIO_CLS_F32_CAPABLE - the
 *   ones whose fp32 cost is < 1 % of a step - are accepted.
 *   SAMAUDIO_OPT_QUANT_CLASSES / SAMAUDIO_OPT_QUANT_FORMAT (fp32 contexts; measurement aid for the error budget of
 *   DESIGN.md section 4): the GEMMs of the named classes round BOTH operands to the 16-bit format (1 = bfloat16,
 *   2 = IEEE fp16) before multiplying, everything else stays exact - the numerical effect of running only that class on
 *   16-bit operands. */
#define SAMAUDIO_OPT_F32_CLASSES 2
#define SAMAUDIO_OPT_QUANT_CLASSES 3
#define SAMAUDIO_OPT_QUANT_FORMAT 4
/*   SAMAUDIO_OPT_ALT16_CLASSES (16-bit contexts; value = mask of the five big GEMM classes of the DiT layers - QKV, WO, CWQ, W13,
 *   W2 -, default 0): precision "mixed".  The named classes read their operands in the library's OTHER 16-bit format - bfloat16
 *   in libsamaudio_hip_f16.so - i.e. BASELINE's dtype for 96 % of the flops, IEEE fp16 for the classes that carry the error
 *   (DESIGN.md section 4); their weight tensors are registered in that format (same dtype code: a 16-bit tensor is bits), and
 *   the kernels that produce their activation operands (RMSNorm + modulate, self-attention, the wo / w13 epilogues) write that
 *   format.  In libsamaudio_hip.so both formats are bfloat16 and the option changes nothing. */
#define SAMAUDIO_OPT_ALT16_CLASSES 5
/*   SAMAUDIO_OPT_PREFETCH_ROWS (16-bit contexts; default 0 = off): in evaluations of at most this many rows (rows = batch x
 *   frames of one samaudio_forward), every big GEMM of a DiT layer that leaves CUs idle (< 256 workgroups: the few-row launches of
 *   a batch shard, 4 clips per GPU) uses them to read the NEXT GEMM's weights once, linearly, so that the next launch finds them
 *   in the memory-side cache instead of fetching them cold.  Scheduling only: results are bitwise unaffected.
 * Weight layout of the five big GEMM classes of the DiT layers (L<i>.wqkv, wo, c_wq, w13, w2), chosen per tensor by the shape it is
 * registered with: [N, K] row-major, or [K/64, N, 64] K-TILE-MAJOR - the 64-element K slab of all N rows contiguous (16-bit contexts
 * only; sam_audio_amd/weights.py ktm_layout).  Same values, same results; a launch of few rows then streams its weights front to back. */
#define SAMAUDIO_OPT_PREFETCH_ROWS 6
/*   SAMAUDIO_OPT_SENTINEL (default 0; validation aid, never on in timed runs): value 1 makes the context scan every 16-bit tensor a
 *   GEMM of the hot path writes (and the RMSNorm / attention outputs that feed GEMMs) for its largest magnitude and for
 *   non-finite values, per GEMM class, on the launch stream - an IEEE-fp16 operand that overflowed (|x| > 65504 -> inf) is then
 *   REPORTED by samaudio_sentinel_read with the class it came from instead of propagating silently.  Non-finite = NaN and +-Inf,
 *   nothing else: every finite value, however large, goes into the magnitude (samaudio_op_sentinel).  Allocates 4 KiB of device
 *   memory on first use (the only allocation of the library besides the checksum trace). */
#define SAMAUDIO_OPT_SENTINEL 7
/* (option 8 was SAMAUDIO_OPT_ODE_GRAPH, rounds 5: a solve's launches replayed as one HIP graph.  Bitwise equal and measured at
 * + 0.0 ... 0.3 % - the host already runs ahead of the GPU, there is no launch gap to close - so it was removed in round 6;
 * profiles/r5_call13/ holds the measurement, the git history the code.) */
/*   SAMAUDIO_OPT_X3_CLASSES (fp32 contexts; value = mask of SAMAUDIO_CLS_X3_CAPABLE bits, default 0): COMPENSATED 16-bit operands -
 *   precision "fp16x3" of the host classes.  The reference computes in fp32 (README.md:48); no plain 16-bit operand format holds
 *   the 1e-3 parity bound on trained-like weight statistics.  A GEMM of a named class keeps its fp32
 *   activation operand and fp32 outputs, but multiplies on the 16-bit MFMA: each operand is split into hi = rn16(x) and
 *   lo = rn16(x - hi), the activation row becomes [lo | hi | hi] (3K elements, written by a streaming kernel on the launch stream)
 *   and the weight row [W_hi | W_lo | W_hi], so that ONE launch of the library's 16-bit GEMM over K' = 3K accumulates
 *   x_lo W_hi + x_hi W_lo + x_hi W_hi in fp32 - the fp32 product to ~2^-21 relative for three times the MFMA work (the 8-phase kernels
 *   know the layout and stage / read what the three products share once: csrc/gemm8.hip gemm8x_kernel).  Needs the
 *   class's weights registered in that split form under "<name>.x3" - 16-bit, [N, 3K] row-major or [3K/64, N, 64] K-tile-major
 *   (sam_audio_amd/weights.py x3_weight) - for L<i>.wqkv, wo, c_wq, c_wo, w13, w2; checked like the ".f32" copies above.  Classes
 *   PATCH (the patcher's k3 convolutions: "patch1.w.x3" / "patch2.w.x3", [D, 9D] with EACH tap's D columns split into 3D) and CKV
 *   ("c_wkv_all.x3") can be switched on as well.  Class CODEC works without a second copy of anything: the fp32 convolution kernel splits
 *   the fp32 fragments of both operands in registers and multiplies them as lo*hi + hi*lo + hi*hi on the 16-bit MFMA.  Optional twins make
 *   it faster: "<name>.x3" ([N, K / Cin, 3 Cin], weights.py convert_codec_x3) sends a convolution with >= 256 output channels through the
 *   16-bit 8-phase kernels over K' = 3K; "<name>.fly" (16-bit, [N, 2K]: the weight split ONCE in the fragment layout of the fp32 kernel,
 *   csrc/common.h GEMM_FLAG_W_FLY16, weights.py convert_codec_fly16) takes the split of the weight out of that kernel's K loop.  Same
 *   bits with or without them.
 *   With class CWO on, text memories of <= 16 tokens (128-wide heads) take the folded form of the cross-attention output projection on
 *   compensated operands (h += P . U, U = Wo V per layer and batch item: K' = 3 * pad64(heads * (8 | 16)) instead of 3 * dim).
 *   Bit SAMAUDIO_X3_ATTENTION does the same for the two contractions of the self-attention.  Everything else of the context
 *   (norms, softmax, the small GEMM classes, the codec) stays exact fp32.  In
 *   libsamaudio_hip_f16.so the halves are IEEE fp16 (22 mantissa bits per operand); in libsamaudio_hip.so bfloat16 (16 bits). */
#define SAMAUDIO_OPT_X3_CLASSES 9
#define SAMAUDIO_SENTINEL_SLOTS 16   /* SAMAUDIO_CLS_COUNT GEMM classes (bit order) + slot 14: RMSNorm outputs, 15: attention outputs */
#define SAMAUDIO_CLS_ALT16_CAPABLE (SAMAUDIO_CLS_QKV | SAMAUDIO_CLS_WO | SAMAUDIO_CLS_CWQ | SAMAUDIO_CLS_W13 | SAMAUDIO_CLS_W2)
#define SAMAUDIO_CLS_TIME (1 << 0)   /* t_embedder MLP + t_block (transformer.py:236-257,462-467): 1 row per time value */
#define SAMAUDIO_CLS_OUT (1 << 1)    /* DiT output projection D -> 256 (transformer.py:519): feeds the ODE state */
#define SAMAUDIO_CLS_IN (1 << 2)     /* proj, noisy-audio columns (model.py:116-125): reads the ODE state */
#define SAMAUDIO_CLS_PREP (1 << 3)   /* hoisted conditioning: proj feature columns, video conv1x1, anchors, memory_proj */
#define SAMAUDIO_CLS_YEMB (1 << 4)   /* y_embedder (transformer.py:260-288) */
#define SAMAUDIO_CLS_CKV (1 << 5)    /* cross-attention K | V projections of all layers */
#define SAMAUDIO_CLS_PATCH (1 << 6)  /* patcher k3 convolutions (patcher.py:48-67) */
#define SAMAUDIO_CLS_QKV (1 << 7)
#define SAMAUDIO_CLS_WO (1 << 8)
#define SAMAUDIO_CLS_CWQ (1 << 9)
#define SAMAUDIO_CLS_CWO (1 << 10)
#define SAMAUDIO_CLS_W13 (1 << 11)
#define SAMAUDIO_CLS_W2 (1 << 12)
#define SAMAUDIO_CLS_CODEC (1 << 13) /* every DAC-VAE convolution */
#define SAMAUDIO_CLS_COUNT 14
/* SAMAUDIO_OPT_X3_CLASSES only (not a GEMM class): the self-attention of an fp32 context on hi/lo-split operands on the 16-bit MFMA
 * (S = Ql Kh + Qh Kl + Qh Kh, O likewise) instead of the fp32 vector-ALU kernel; fp32 tensors in and out */
#define SAMAUDIO_X3_ATTENTION (1 << 14)
#define SAMAUDIO_CLS_X3_CAPABLE \
  (SAMAUDIO_CLS_QKV | SAMAUDIO_CLS_WO | SAMAUDIO_CLS_CWQ | SAMAUDIO_CLS_CWO | SAMAUDIO_CLS_W13 | SAMAUDIO_CLS_W2 | SAMAUDIO_CLS_PATCH | \
   SAMAUDIO_CLS_CKV | SAMAUDIO_CLS_CODEC | SAMAUDIO_X3_ATTENTION)
/* the bits samaudio_judge_set_option / samaudio_frame_set_option accept (the PE-AV towers, see there) */
#define SAMAUDIO_CLS_X3_TOWER \
  (SAMAUDIO_CLS_QKV | SAMAUDIO_CLS_WO | SAMAUDIO_CLS_W13 | SAMAUDIO_CLS_W2 | SAMAUDIO_CLS_PATCH | SAMAUDIO_X3_ATTENTION)
/* the bits samaudio_vit_set_option accepts (the PE-Core vision tower, see there) */
#define SAMAUDIO_CLS_X3_VIT (SAMAUDIO_CLS_QKV | SAMAUDIO_CLS_WO | SAMAUDIO_CLS_W13 | SAMAUDIO_CLS_W2 | SAMAUDIO_X3_ATTENTION)
#define SAMAUDIO_CLS_F32_CAPABLE (SAMAUDIO_CLS_TIME | SAMAUDIO_CLS_OUT | SAMAUDIO_CLS_IN | SAMAUDIO_CLS_PREP | SAMAUDIO_CLS_YEMB)
int samaudio_set_option(samaudio_ctx* ctx, int option, int value);

/* ---- hot path ------------------------------------------------------------------------------------ */

/* Everything of SAMAudio.forward that does not depend on (noisy_audio, time): the audio_features / video /
 * anchor terms of align_inputs (model.py:108-128, align.py:30-50, model.py:54-65) and memory_proj(text)
 * (model.py:171).  rows = B * candidates (conditioning already repeated, model.py:193-229).
 *   audio_features [rows, frames, 256] f32      text [rows, text_len, text_dim] f32 or NULL
 *   text_mask      [rows, text_len] u8 or NULL  video [rows, frames, video_dim] f32 (channels-last) or NULL
 *   anchor_ids     [rows, n_ids] i64 or NULL    anchor_alignment [rows, frames] i64
 *   audio_pad_mask [rows, frames] u8 or NULL (1 = valid frame)                                          */
int samaudio_prepare(samaudio_ctx* ctx, int rows, int frames, int text_len, const float* audio_features,
                     const float* text, const uint8_t* text_mask, const float* video, const int64_t* anchor_ids,
                     int n_ids, const int64_t* anchor_alignment, const uint8_t* audio_pad_mask,
                     samaudio_stream stream);
/* The same with the conditioning as separate() holds it (no concatenated / repeated copies):
 *   latent [rows / candidates, frames, latent_channels / 2] f32: the DAC-VAE mean latent z; audio_features = (z | z)
 *   (model.py:182-184) is never materialised - the feature GEMM reads each z row twice (two K taps, stride 0);
 *   candidates >= 1: text / text_mask / video / anchor_ids / anchor_alignment / audio_pad_mask hold rows / candidates clips; the
 *   per-clip conditioning is computed once and repeated sample-major for the clip's candidates (model.py:193-203) inside the engine. */
int samaudio_prepare_latent(samaudio_ctx* ctx, int rows, int frames, int text_len, int candidates, const float* latent,
                            const float* text, const uint8_t* text_mask, const float* video, const int64_t* anchor_ids,
                            int n_ids, const int64_t* anchor_alignment, const uint8_t* audio_pad_mask, samaudio_stream stream);

/* One ODE function evaluation = SAMAudio.forward (model.py:130-180) -> DiT.forward (transformer.py:473-524).
 *   noisy [rows, frames, 256] f32, time [n_time] f32 with n_time in {1, rows}, out [rows, frames, 256] f32 */
int samaudio_forward(samaudio_ctx* ctx, const float* noisy, const float* time, int n_time, float* out,
                     samaudio_stream stream);

/* Fixed-grid ODE solve, replaces torchdiffeq.odeint at model.py:285-290 (method SAMAUDIO_ODE_*: "euler" | "midpoint" | "rk4" |
 * "heun3").  grid_host: n_grid strictly increasing time points on the HOST (t0 .. t1); state [rows, frames, 256] f32 is updated
 * in place from the noise to states[-1].  The evaluation times of a solve are handed to the device as kernel arguments into a
 * table of 4096 floats: midpoint and euler take 2 * n_grid of them, rk4 / heun3 one per stage and step (4 resp. 3 * (n_grid - 1));
 * a longer grid is SAMAUDIO_ERR_ARG.  rk4 / heun3 need the context's stage buffers (below): missing or too small =
 * SAMAUDIO_ERR_WORKSPACE; a library built without ode_stage_kernel (the CPU launcher emulation) refuses them with
 * SAMAUDIO_ERR_STATE. */
int samaudio_ode_solve(samaudio_ctx* ctx, float* state, int method, const float* grid_host, int n_grid,
                       samaudio_stream stream);
/* Stage buffers of the Runge-Kutta methods, borrowed from the caller like the workspace and apart from it (the workspace plan, and
 * so samaudio_workspace_bytes, is the same for every method): one fp32 array of rows * frames * 256 elements per stage, each on a
 * 256-byte boundary.  samaudio_ode_stage_bytes = what a solve of `method` over [rows, frames] needs (0 for euler and midpoint,
 * which use none).  samaudio_set_ode_stages hands the context its buffer (256-byte aligned; NULL withdraws it); it must not overlap
 * the workspace or the state, and each context of a process needs its own. */
size_t samaudio_ode_stage_bytes(samaudio_ctx* ctx, int method, int rows, int frames);
int samaudio_set_ode_stages(samaudio_ctx* ctx, void* stages, size_t bytes);

/* Adaptive ODE solve with PER-ROW step control (tests/ode_adaptive_ref.py is the statement).  method
 * SAMAUDIO_ODE_DOPRI5 (Dormand-Prince 5(4): 6 evaluations per trial step) | SAMAUDIO_ODE_BOSH3 (Bogacki-Shampine 3(2): 3), both FSAL.
 * Every row of state [rows, frames, 256] f32 integrates from t0 to t1 on its own: its time, its step, its error norm - the root mean
 * square of h K^T E / (atol + rtol max(|y|, |y_new|)) over the row's valid frames (the audio_pad_mask of samaudio_prepare) and all
 * channels - and its accept / reject decision live on the device, so a row's result does not depend on which rows share the call.
 * Tableaux, controller and initial step are those of scipy.integrate's RK45 / RK23 (max_step = inf) in fp32; pinned to scipy,
 * unpinned vs torchdiffeq, from which it departs in that the norm and the step are per row, the last step is clipped to end at t1
 * exactly, and the accept factor is capped at 1 after a rejection within the same step.
 * UNLIKE samaudio_ode_solve THIS CALL SYNCHRONISES THE STREAM, once per trial step: the host has to learn whether a row is still
 * running.  Rows that have ended ride along, untouched, until the last one ends.
 * The context's stage buffers (samaudio_ode_stage_bytes answers for these methods: the K rows, the candidate state, the per-row
 * control block, the per-stage time table and the norm partials) are the caller's as for rk4: missing or too small or overlapping =
 * SAMAUDIO_ERR_WORKSPACE with the state untouched; a library built without the kernels (the CPU launcher emulation) = SAMAUDIO_ERR_STATE;
 * a window table set (samaudio_set_windows) without a group table = SAMAUDIO_ERR_STATE; with one (samaudio_set_window_groups) the
 * unit of step control is the group, not the row.  stats_host: HOST array, one entry per row.  A row that fails (status
 * 2: a rejection drove its step below 10 ulp(t); 3: max_num_steps trial steps) stops where it is while the other rows go on; the call
 * still returns SAMAUDIO_OK and the caller reads the status. */
typedef struct {
  float rtol, atol;         /* > 0 */
  float first_step;         /* <= 0: scipy's select_initial_step (one more field evaluation) */
  float safety;             /* 0.9  */
  float ifactor;            /* 10: the largest growth of a step  */
  float dfactor;            /* 0.2: the largest shrink after a rejection */
  int32_t max_num_steps;    /* trial steps (accepted + rejected) a row may take */
} samaudio_ode_adaptive;
enum { SAMAUDIO_ODE_ROW_RUNNING = 0, SAMAUDIO_ODE_ROW_FINISHED = 1, SAMAUDIO_ODE_ROW_STEP_UNDERFLOW = 2, SAMAUDIO_ODE_ROW_MAX_STEPS = 3 };
typedef struct {
  int32_t accepted, rejected;   /* steps of this row */
  int32_t status;               /* SAMAUDIO_ODE_ROW_* */
  int32_t evaluations;          /* field launches of the whole solve (the same in every entry) */
  float t, last_h;              /* where the row stands (t1 exactly when finished), its last accepted step */
} samaudio_ode_row_stats;
int samaudio_ode_solve_adaptive(samaudio_ctx* ctx, float* state, int method, float t0, float t1, const samaudio_ode_adaptive* opt,
                                samaudio_ode_row_stats* stats_host, samaudio_stream stream);

/* Windowed solve of clips longer than one window (SAMAudio.separate(window_seconds=...)).  The prepared rows
 * are windows of `frames` frames cut from longer clips with a stride of frames - overlap_frames; next_row_device [rows] i32 ON THE
 * DEVICE names for every row the row that holds the clip's next window, or -1.  While a table is set, every field evaluation
 * (samaudio_forward, every stage of every samaudio_ode_solve method) ends with one launch of window_blend_kernel on its output: for a
 * row r with successor s, frame j < overlap_frames of the overlap becomes v = p + a_j (q - p), p = out[r, frames - overlap + j],
 * q = out[s, j], a_j = (j + 1) / (overlap + 1), written to BOTH places - so rows whose overlapping frames start equal stay equal, bit
 * for bit, through the whole solve.  Call it after samaudio_prepare / samaudio_prepare_latent: rows must be the prepared row count and
 * 1 <= overlap_frames <= frames / 2 (SAMAUDIO_ERR_ARG otherwise; SAMAUDIO_ERR_STATE before any prepare).  The table is borrowed until
 * it is replaced; its contents are the caller's responsibility (the host cannot read them without a blocking copy) - an entry outside
 * [0, rows) or equal to its own index counts as -1, two rows naming the same successor is undefined.  next_row_device = NULL switches
 * windows off, and so does every later samaudio_prepare / samaudio_prepare_latent: a stale table never meets a new batch.  A library
 * built without the kernel (the CPU launcher emulation) answers SAMAUDIO_ERR_STATE. */
int samaudio_set_windows(samaudio_ctx* ctx, const int32_t* next_row_device, int rows, int overlap_frames);
/* Step control PER CLIP for samaudio_ode_solve_adaptive over window rows (tests/ode_windowed_adaptive_ref.py
 * is the statement).  groups_device [n_groups, 3] i32 ON THE DEVICE: first engine row, window count, row stride of each group - the
 * window rows of one (clip, candidate); owner_mask_device [rows, frames] u8 ON THE DEVICE: 1 where the row OWNS the frame - the frame
 * is valid and lies before the stride (frames - overlap), or the row is its clip's last window - so every valid frame of a clip is
 * owned by exactly one row.  While both are set, an adaptive solve carries one time, one step, one error norm (over the group's owned
 * frames, each counted once: partials added in window order, chunk order within a row) and one accept / reject decision per group,
 * written identically to every row of the group; a clip's result then does not depend on which clips share the call.
 * Valid only after samaudio_set_windows (SAMAUDIO_ERR_STATE otherwise); n_groups outside [1, rows], a null mask or a misaligned
 * table = SAMAUDIO_ERR_ARG.  Both arrays are borrowed until replaced; their contents are the caller's responsibility - a row index
 * outside [0, rows) counts as absent, rows in no group are not stepped.  groups_device = NULL clears them, and so do
 * samaudio_set_windows (NULL or not) and every samaudio_prepare / samaudio_prepare_latent. */
int samaudio_set_window_groups(samaudio_ctx* ctx, const int32_t* groups_device, int n_groups, const uint8_t* owner_mask_device);
/* kernel-level hook: the blend above on out [rows, frames, channels] f32 in place.  SAMAUDIO_ERR_ARG before any launch for a null
 * pointer, rows < 1, frames < 2, overlap outside [1, frames / 2], channels % 4 != 0, out not aligned to 16 bytes. */
int samaudio_op_window_blend(float* out, const int32_t* next_row, int rows, int frames, int overlap, int channels,
                             samaudio_stream stream);

/* DAC-VAE.  encode (codec.py:65-70): wav [items, samples] f32, samples % hop == 0 -> mean latent
 * [items, samples/hop, codec_dim] f32 (channels-last).  decode (codec.py:86-89):
 * latent [items, frames, codec_dim] f32 (channels-last) -> wav [items, frames*hop] f32. */
int samaudio_codec_encode(samaudio_ctx* ctx, const float* wav, int items, int64_t samples, float* latent,
                          samaudio_stream stream);
int samaudio_codec_decode(samaudio_ctx* ctx, const float* latent, int items, int frames, float* wav,
                          samaudio_stream stream);
/* Decode straight from the ODE state (reference model.py:291-295 without the transposed copy): state [rows, frames, 2 * codec_dim]
 * f32 -> wav [2 * rows, frames * hop]: waveform 2b = channels [0, codec_dim) of row block b (target), 2b + 1 the rest (residual). */
int samaudio_codec_decode_pairs(samaudio_ctx* ctx, const float* state, int rows, int frames, float* wav, samaudio_stream stream);

/* The same three in time tiles (no reference counterpart).  The codec is a stack of convolutions: a latent
 * frame depends on samaudio_codec_halo_frames(ctx, decode) frames of input either side of it and no more (the reach, derived from the
 * layers the engine launches, rounded up to whole frames).  Tile k of `tile_frames` = L frames is one pass over frames
 * [max(0, kL - h), min(T, (k + 1) L + h)) of every item that writes rows [kL, min(T, (k + 1) L)) only, straight into the caller's
 * tensor; T = frames (samples / hop) is the padded length, as in the whole pass.  Results equal the untiled call's bit for bit.
 * The workspace a call needs is samaudio_workspace_bytes(ctx, 0, 0, 0, items_per_pass, samaudio_codec_tile_samples(ctx, frames,
 * tile_frames, decode)): it does not grow with the clip (tile_samples: the longest segment in samples; < 0 when frames or
 * tile_frames < 1).  tile_frames >= frames is the untiled call, launch for launch.  tile_frames < 1: SAMAUDIO_ERR_ARG; a workspace
 * too small for one segment of one item (of one pair): SAMAUDIO_ERR_WORKSPACE. */
int samaudio_codec_halo_frames(samaudio_ctx* ctx, int decode);
int64_t samaudio_codec_tile_samples(samaudio_ctx* ctx, int frames, int tile_frames, int decode);
int samaudio_codec_encode_tiled(samaudio_ctx* ctx, const float* wav, int items, int64_t samples, int tile_frames, float* latent,
                                samaudio_stream stream);
int samaudio_codec_decode_tiled(samaudio_ctx* ctx, const float* latent, int items, int frames, int tile_frames, float* wav,
                                samaudio_stream stream);
int samaudio_codec_decode_pairs_tiled(samaudio_ctx* ctx, const float* state, int rows, int frames, int tile_frames, float* wav,
                                      samaudio_stream stream);

/* ---- reranking and span prediction ------------------------------------------ */

/* One PE-AV transformer (perception_models core.audio_visual_encoder.transformer.Transformer, un-vendored; the
 * reference instantiates it at sam_audio/model/judge.py:46-47; restated from its Hugging Face port
 * transformers/models/pe_audio/modeling_pe_audio.py:241-287,344-490,616-680). */
typedef struct {
  int32_t dim, n_heads, n_layers, ffn_hidden; /* hidden_size, num_attention_heads, num_hidden_layers, intermediate_size */
  int32_t in_dim;                             /* width of the features entering the input projection */
  int32_t max_positions;                      /* rows of the RoPE table */
  int32_t attn_bias;                          /* 1: q/k/v/o projections carry biases */
  float norm_eps;
} samaudio_peav_dims;

/* SAMAudioJudgeModel (reference sam_audio/model/judge.py:35-132, config.py:234-251).  The ModernBERT text tower and
 * the tokenizer stay with the caller (PyTorch-ROCm); the DAC encoder is a codec-only samaudio_ctx. */
typedef struct {
  int32_t precision;
  samaudio_peav_dims transformer, finetune_transformer;
  int32_t codec_dim;      /* 128: transformer.in_dim */
  int32_t text_hidden;    /* text_model.hidden_size */
  int32_t bottleneck_dim; /* 256: finetune_transformer.in_dim */
} samaudio_judge_config;

typedef struct samaudio_judge samaudio_judge;
int samaudio_judge_create(const samaudio_judge_config* cfg, samaudio_judge** out);
void samaudio_judge_destroy(samaudio_judge* j);
/* engine names: sam_audio_amd/judge.py documents the mapping from the reference state_dict keys */
int samaudio_judge_set_tensor(samaudio_judge* j, const char* name, const void* data, int dtype, int ndim,
                              const int64_t* shape);
/* SAMAUDIO_OPT_X3_CLASSES for the PE-AV towers (fp32 contexts only; set it BEFORE samaudio_judge_finalize, which resolves the twins;
 * query the workspace after it): value = mask of SAMAUDIO_CLS_X3_TOWER bits, 0 (default) = the exact-fp32 launches.  Per transformer:
 *   QKV / WO / W13 / W2   the four GEMMs of every layer as 16-bit launches over K' = 3K on "<prefix>L<i>.<name>.x3"
 *                         ([N, 3K] = [W_hi | W_lo | W_hi], or K-tile-major [3K/64, N, 64]); QKV / W13 also need the norm in front
 *                         as a constant table "<prefix>L<i>.attn_norm.gs" / ".ffn_norm.gs" [2, dim] f32 = [gain | zeros];
 *                         WO also switches the output projection ("<prefix>out.w.x3", "<prefix>norm.gs") and, in a Judge, both halves of
 *                         cat_audio_proj ("cat.wh.x3", "cat.wi.x3": K = dim over every frame)
 *   PATCH                 the two k3 convolutions of the ResNet block on "<prefix>conv<n>.w.x3" [dim, 3 taps x 3 dim] (each tap's
 *                         columns split on their own, like patch1.w.x3)
 *   SAMAUDIO_X3_ATTENTION the self-attention's two contractions on split operands
 * The input projections, the Judge's text branch and proj_audio_and_text, the span predictor's heads (K <= 256, or one row per
 * pair) stay exact fp32.  Any other bit, or a 16-bit context: SAMAUDIO_ERR_ARG.  A twin that is missing: SAMAUDIO_ERR_WEIGHT from
 * finalize, naming it. */
int samaudio_judge_set_option(samaudio_judge* j, int option, int value);
int samaudio_judge_finalize(samaudio_judge* j);
size_t samaudio_judge_workspace_bytes(samaudio_judge* j, int inputs, int candidates, int frames);
int samaudio_judge_set_workspace(samaudio_judge* j, void* workspace, size_t bytes);
/* SAMAudioJudgeModel.forward after the codec and the text tower (judge.py:98-132):
 *   input_latent     [inputs, frames, codec_dim] f32              DAC mean latents of the mixtures (codec.py:65-70)
 *   separated_latent [inputs*candidates, frames, codec_dim] f32   ... of the candidate separations, sample-major
 *   text_pooled      [inputs*candidates, text_hidden] f32         _get_text_output(...).pooler_output (judge.py:76-88)
 *   pad_mask         [inputs, frames] u8 or NULL                  padding_mask[:, ::hop] (judge.py:104-107), 1 = valid
 *   scores           [inputs*candidates, 4] f32                   overall, recall, precision, faithfulness (de-normalised)
 * The reference repeats every mixture once per candidate (ranking/judge.py:31-33); all ops are per-row, so the
 * mixture branch runs once per clip here.  candidates = 1 is the plain forward(). */
int samaudio_judge_score(samaudio_judge* j, const float* input_latent, const float* separated_latent, int inputs,
                         int candidates, int frames, const float* text_pooled, const uint8_t* pad_mask, float* scores,
                         samaudio_stream stream);
/* parity hook: transformer `which` (0 = transformer, 1 = finetune_transformer) alone:
 * x [rows, frames, in_dim] f32 -> hidden [rows, frames + 1, dim] f32 (row 0 of each item = pooler_output). */
int samaudio_judge_encode(samaudio_judge* j, int which, const float* x, const uint8_t* pad_mask, int rows, int frames,
                          float* hidden, samaudio_stream stream);

/* PE-A-Frame span predictor (reference model.py:96-102,231-245; un-vendored PEAudioFrame; Hugging Face port
 * modeling_pe_audio.py:810-868): per-frame audio-text logits for batch-paired (audio, description) rows. */
typedef struct {
  int32_t precision;
  samaudio_peav_dims audio;
  int32_t codec_dim;  /* 128 */
  int32_t embed_dim;  /* text hidden size = width of the joint space */
} samaudio_frame_config;

typedef struct samaudio_frame samaudio_frame;
int samaudio_frame_create(const samaudio_frame_config* cfg, samaudio_frame** out);
void samaudio_frame_destroy(samaudio_frame* f);
int samaudio_frame_set_tensor(samaudio_frame* f, const char* name, const void* data, int dtype, int ndim,
                              const int64_t* shape);
int samaudio_frame_set_option(samaudio_frame* f, int option, int value);   /* as samaudio_judge_set_option (prefix "a.") */
int samaudio_frame_finalize(samaudio_frame* f);
size_t samaudio_frame_workspace_bytes(samaudio_frame* f, int rows, int frames);
int samaudio_frame_set_workspace(samaudio_frame* f, void* workspace, size_t bytes);
/* codec_features [rows, frames, codec_dim] f32 (= audio_features[:, :, :128], model.py:239), text_pooled
 * [rows, embed_dim] f32 (token 0 of the text tower's last hidden state), pad_mask [rows, frames] u8 or NULL
 * -> logits [rows, frames] f32 */
int samaudio_frame_logits(samaudio_frame* f, const float* codec_features, const float* text_pooled,
                          const uint8_t* pad_mask, int rows, int frames, float* logits, samaudio_stream stream);

/* ---- visual-prompt tower -------------------------------------------------------
 * PE-Core vision tower behind `PerceptionEncoder.encode` (reference sam_audio/model/vision_encoder.py:80-89:
 * `pe.CLIP.from_config("PE-Core-L14-336")`, `encode_image(x, normalize=...)`).  samaudio_vit_encode takes frames the caller has
 * resized, scaled and normalised (vision_encoder.py:91-113) and runs everything from the patch embedding to the L2-normalised
 * feature; samaudio_vit_encode_frames takes the raw uint8 frames and does the resize, the rounding and the normalisation as
 * well, in the launch that writes the patch embedding's operand.  Engine tensor names: sam_audio_amd/vision_tower.py documents
 * the mapping from the `visual.*` state_dict keys. */
typedef struct {
  int32_t precision;                          /* SAMAUDIO_F32 | SAMAUDIO_BF16 */
  int32_t image_size, patch_size;             /* 336, 14 */
  int32_t width, layers, heads, mlp_width;    /* 1024, 24, 16 (head dim 64 or 128), 4096 */
  int32_t output_dim;                         /* 1024 */
  int32_t use_cls_token, use_rope2d, use_ln_pre, use_ln_post;
  int32_t pool_type;                          /* 0 = class token, 1 = token mean, 2 = attention pooling */
  int32_t pool_heads;                         /* heads of the pooling attention (8; head dim 64 or 128) */
  int32_t act;                                /* 4 = GELU (erf), 5 = quick GELU */
  float ln_eps;
} samaudio_vit_config;

typedef struct samaudio_vit samaudio_vit;
int samaudio_vit_create(const samaudio_vit_config* cfg, samaudio_vit** out);
void samaudio_vit_destroy(samaudio_vit* v);
int samaudio_vit_set_tensor(samaudio_vit* v, const char* name, const void* data, int dtype, int ndim,
                            const int64_t* shape);
/* SAMAUDIO_OPT_X3_CLASSES for the vision tower - the only option it takes (fp32 contexts only; set it BEFORE samaudio_vit_finalize, which
 * resolves the twins; query the workspace after it): value = mask of SAMAUDIO_CLS_X3_VIT bits, 0 (default) = the exact-fp32 launches,
 * bit for bit what a context that never set the option computes.  Per layer:
 *   QKV                   L<i>.wqkv as one 16-bit launch over K' = 3K on "L<i>.wqkv.x3" ([3W, 3W] = [W_hi | W_lo | W_hi], or K-tile-major
 *                         [3K/64, N, 64]); the LayerNorm in front writes the split rows [lo | hi | hi] itself.  The same bit switches the
 *                         pooling head's k|v projection of every token ("pool.wkv.x3" [2W, 3W])
 *   WO                    "L<i>.wo.x3" [W, 3W]
 *   W13                   the c_fc projection (bias + GELU / quick GELU) on "L<i>.w1.x3" [F, 3W]; with W2 on as well its epilogue writes
 *                         c_proj's operand in split form where the 8-phase family takes the launch
 *   W2                    "L<i>.w2.x3" [W, 3F]
 *   SAMAUDIO_X3_ATTENTION the self-attention's two contractions on split operands (head width 64 or 128)
 * What stays exact fp32, like the small launches of the PE-AV towers: the patch embedding (0.2 % of the flops, a batched launch with a
 * row offset), ln_pre, the pooling attention itself, every launch of one row per frame (pool.wo, pool.w1, pool.w2, proj) and the L2
 * normalisation.  Any other option or bit, or a 16-bit context: SAMAUDIO_ERR_ARG.  A twin that is missing: SAMAUDIO_ERR_WEIGHT from
 * finalize, naming it.  Setting the option marks the context as not finalized, as samaudio_vit_set_tensor does. */
int samaudio_vit_set_option(samaudio_vit* v, int option, int value);
int samaudio_vit_finalize(samaudio_vit* v);
/* Scratch of `frames` frames per encode; with SAMAUDIO_OPT_X3_CLASSES also the split operands of the classes that are on (tokens * 3 *
 * width 16-bit elements for QKV / WO / W13, tokens * 3 * mlp_width for W2): query it AFTER setting the option. */
size_t samaudio_vit_workspace_bytes(samaudio_vit* v, int frames);
int samaudio_vit_set_workspace(samaudio_vit* v, void* workspace, size_t bytes);
/* frames [n, 3, image_size, image_size] f32 (resized, scaled, normalised) -> features [n, output_dim] f32, L2-normalised
 * when `normalize` != 0.  tokens_out (nullable, parity hook): the residual stream after the last block,
 * [n, tokens, width] f32 (before ln_post). */
int samaudio_vit_encode(samaudio_vit* v, const float* frames, int n, int normalize, float* features, float* tokens_out,
                        samaudio_stream stream);
/* Resize of uint8 frames to a square target, as torch's F.interpolate(x.float(), (S, S), mode, antialias=True, align_corners=False)
 * (NEAREST: mode="nearest") followed by round-half-to-even, clamp to 0..255 and (v / 255 - 0.5) / 0.5.  Per axis with `in` source
 * pixels and `out` = S: scale = in / out, support = max(scale, 1) * r (r = 2 bicubic, 1 bilinear), inv = 1 / max(scale, 1); output i:
 * c = scale (i + 0.5), taps lo = max(0, int(c - support + 0.5)) .. hi = min(in, int(c + support + 0.5)) with weights
 * f((s - c + 0.5) inv) normalised to sum 1, f = the triangle filter | the cubic convolution filter with a = -0.5; the horizontal
 * pass, then the vertical pass, accumulated in fp32.  NEAREST: source min(floor(i * (float)in / (float)out), in - 1). */
#define SAMAUDIO_RESIZE_NEAREST  0
#define SAMAUDIO_RESIZE_BILINEAR 1
#define SAMAUDIO_RESIZE_BICUBIC  2
/* kernel-level hook: frames [n,3,height,width] u8 -> out [n,3,out_size,out_size] f32, resized, rounded, normalised.
 * SAMAUDIO_ERR_STATE in a build of the library without the kernel. */
int samaudio_op_resize_frames(const uint8_t* frames, int n, int height, int width, int out_size, int mode,
                              float* out, samaudio_stream stream);
/* samaudio_vit_encode on raw frames [n, 3, height, width] u8 (any height, width >= 1; frames that already have the target size take
 * the same path): the resize writes the patch-embedding operand itself - no float copy of the source and no resized image in memory;
 * everything behind it is samaudio_vit_encode's, bit for bit what it computes from samaudio_op_resize_frames' output.  Same workspace
 * (samaudio_vit_workspace_bytes is unchanged).  A null pointer, n <= 0, height / width < 1 or an unknown mode: SAMAUDIO_ERR_ARG. */
int samaudio_vit_encode_frames(samaudio_vit* v, const uint8_t* frames, int n, int height, int width, int mode,
                               int normalize, float* features, float* tokens_out, samaudio_stream stream);
/* The visual prompt without its two host passes (reference sam_audio/processor.py:147-153, 197-204: `v * m.eq(0)` over the whole video,
 * then `video[idx]`): samaudio_op_resize_frames on n frames PICKED from a video, MASKED while they are read.  frames
 * [src_frames, 3, height, width] u8; output frame f is computed from source frame pick[f] (`pick`: device array of n i32; NULL = the
 * identity, n must then equal src_frames).  The table is built and range-checked by the caller on the host; the kernel clamps every
 * entry into [0, src_frames), so a bad table reads a wrong frame, never outside the tensors.  mask [src_frames, mask_channels, height,
 * width] u8 (bool storage included), mask_channels = 1 (one plane for the three channels) or 3: a source pixel counts as 0 where its
 * mask byte is non-zero; NULL = no mask, mask_channels is then ignored.  The masked value 0 goes through the same taps in the same
 * order with the same weights: out [n, 3, out_size, out_size] f32 is bit-identical to samaudio_op_resize_frames on
 * (frames * (mask == 0))[pick] materialised.  Neither pointer needs any alignment.  SAMAUDIO_ERR_ARG before any launch for a null
 * frames / out, src_frames / n / height / width / out_size < 1, mask_channels not 1 or 3 with a mask, an unknown mode, or pick == NULL
 * with n != src_frames; SAMAUDIO_ERR_STATE in a build of the library without the kernel. */
int samaudio_op_resize_video(const uint8_t* frames, int64_t src_frames, int height, int width, const uint8_t* mask,
                             int mask_channels, const int32_t* pick, int n, int out_size, int mode, float* out,
                             samaudio_stream stream);
/* samaudio_vit_encode_frames on such a video: the picked, masked frames exist only as the patch-embedding operand; everything behind
 * that launch is samaudio_vit_encode's, so features (and tokens_out) are bit for bit what samaudio_vit_encode_frames computes from the
 * materialised frames.  Same workspace, sized for the n picked frames (samaudio_vit_workspace_bytes(n) is unchanged).  Errors as
 * samaudio_op_resize_video (features in the place of out), checked before the context's state. */
int samaudio_vit_encode_video(samaudio_vit* v, const uint8_t* frames, int64_t src_frames, int height, int width,
                              const uint8_t* mask, int mask_channels, const int32_t* pick, int n, int mode, int normalize,
                              float* features, float* tokens_out, samaudio_stream stream);

/* ---- audio front end: resample, mix down and pad one PCM clip ------------------------------
 * What the reference does with torchaudio before batching (sam_audio/processor.py:23-36: load, functional.resample, mean over
 * channels, right zero padding), as one kernel per clip.  The resampler is the band-limited Hann-windowed sinc interpolation of
 * sam_audio_amd/processor.py resample, which stays the CPU statement.  With g = gcd(orig, new), o = orig / g (`step`), n = new / g
 * (`phases`), base = min(o, n) rolloff, width = ceil(lw o / base):
 *     y[j] = sum_d h(p, d) x[f o + d],   f = j / n,  p = j % n,  d in [-width, width + o),  x = 0 outside [0, samples),
 *            j < ceil(n samples / o)
 *     h(p, d) = sinc(pi t) cos^2(pi t / (2 lw)) base / o,   t = clamp((d / o - p / n) base, -lw, lw),  sinc(0) = 1
 * Rounded to fp32 the non-zero weights of a phase form one run; the caller hands the runs over in compact form
 * (sam_audio_amd/audio.py filter_bank): first [phases] i32 = the d of each phase's first tap, taps [taps_per_phase][phases] f32
 * (tap-major: taps[t * phases + p] weighs x[f o + first[p] + t]; zeros behind a run).  x is the mean over the channels, taken before
 * the filter; every output sums its taps in ascending d in fp32 (one fma per tap), so sample j does not depend on the launch geometry,
 * on out_capacity or on other clips.  Same rate = (phases, step, taps_per_phase) = (1, 1, 1), first = {0}, taps = {1}: convert, mix, pad.
 * pcm: element (c, i) at pcm[c * ch_stride + i * s_stride] (strides in elements: interleaved frames = (1, channels), planar =
 * (samples, 1)), aligned to its element size only; S16 values are scaled by exactly 1 / 32768. */
#define SAMAUDIO_PCM_S16 0
#define SAMAUDIO_PCM_F32 1
/* ceil(phases * samples / step): the length of a resampled clip; -1 when an argument is below 1 */
int64_t samaudio_resample_length(int64_t samples, int step, int phases);
/* out[0, length) = the resampled mono mix, out[length, out_capacity) = 0; nothing is written behind out_capacity.  Stateless, like
 * samaudio_op_resize_frames.  SAMAUDIO_ERR_ARG before any launch for a null pointer, channels / samples / step / phases /
 * taps_per_phase < 1, an unknown format or out_capacity < length; SAMAUDIO_ERR_STATE in a build of the library without the kernel. */
int samaudio_op_resample(const void* pcm, int fmt, int channels, int64_t samples, int64_t ch_stride, int64_t s_stride,
                         const float* taps, const int32_t* first, int phases, int step, int taps_per_phase, float* out,
                         int64_t out_capacity, samaudio_stream stream);

/* ---- sound activity: silence detection and span overlap of `rows` mono waveforms -----------
 * The reference's SoundActivityRanker (sam_audio/ranking/sound_activity.py): pydub.silence.detect_nonsilent on the separated
 * waveform, then compute_iou_recall_precision against the prompt's spans.  The CPU statement is tests/activity_ref.py - pinned to
 * CPython's audioop (what pydub calls), unpinned vs pydub / torchcodec.  All of it is integer arithmetic behind step 1:
 *   1  s = clip(rint(fp64(x) 32768), -32768, 32767) as int16, round half to even, NaN -> 0
 *   2  to 24 kHz as audioop.ratecv does: i = rate / g (`step`), o = 24000 / g (`phases`), g = gcd, M input samples,
 *      N = floor(o (M - 1) / i) + 1;  m = ceil(i j / o), d = o m - i j,  y[j] = trunc(65536 (s[m-1] d + s[m] (o - d)) / o) >> 16,  s[-1] = 0
 *   3  L = round(1000 N / 24000) ms, ties to even.  A slice [a, b) ms is frames [24 a, 24 b), frames at or beyond N count as zero
 *   4  S(i) = sum of y^2 over the 6 000 frames of the window that starts at i ms;  rms(i) = floor(sqrt(S(i) / 6000))
 *   5  L < 250: the nonsilent spans are [[0, L]]
 *   6  peak = max rms(i), i in range(0, L - 250 + 1, 100)
 *   7  thresh(peak): "rel_to_max" 10^((sil_threshold + 20 log10(peak / 32768)) / 20) 32768, "abs" 10^(sil_threshold / 20) 32768.  The
 *      caller evaluates it on the host for every peak in [0, 32768] and hands over threshold_table[peak] = min(floor(thresh), 65535):
 *      rms(i) <= thresh  <=>  S(i) < (T + 1)^2 6000.  No logarithm or power is evaluated on the device.
 *   8  window starts range(0, L - 250 + 1, 10), plus L - 250 when (L - 250) % 10 != 0; a start is silent iff rms(i) <= thresh
 *   9  silent ranges (detect_silence): walk the silent starts; close the range at prev + 250 when the next start is neither
 *      prev + 10 nor <= prev + 250; close the last one
 *  10  nonsilent ranges (detect_nonsilent): no silent range -> [[0, L]]; the gaps from 0 on, a final [prev_end, L] unless the last
 *      silent range ends at L, a leading [0, 0] dropped; at most L / 250 + 1 of them.  In seconds: ms / 1000 in float64
 *  11  score = iou | recall | precision (metric 0 | 1 | 2) of compute_iou_recall_precision(nonsilent spans, ref_spans), float64 in
 *      the reference's order of operations (overlapping reference spans count twice, as there), rounded to float32
 * wav: row r at wav + r * row_stride, contiguous in time.  The same ref_spans [n_ref][2] (seconds, f64, device) for every row. */
/* L of step 3; -1 for an argument below 1 or phases not a divisor of 24 000 */
int64_t samaudio_activity_length_ms(int64_t samples, int step, int phases);
/* bytes of workspace samaudio_op_activity needs (rows x max(L, 1) int64, aligned to 8); -1 as above or for rows < 1 */
int64_t samaudio_activity_workspace_bytes(int rows, int64_t samples, int step, int phases);
/* scores [rows] f32; and, each where not NULL, spans [rows][max_spans][2] i32 = (start_ms, end_ms) of the first span_count [rows]
 * nonsilent spans (the rest of a row is left as it was) and peak [rows] (0 when L < 250).  ref_spans NULL or n_ref = 0: spans only,
 * scores 0.  Stateless, caller workspace, nothing is read back.  SAMAUDIO_ERR_ARG before any launch for a null wav /
 * threshold_table / workspace / scores, rows / samples / step / phases < 1, phases not a divisor of 24 000, row_stride < samples, a
 * metric outside 0..2, n_ref < 0 or n_ref > 0 with null ref_spans, a workspace that is too small or not aligned to 8 bytes, spans
 * with max_spans < L / 250 + 1; SAMAUDIO_ERR_STATE in a build of the library without the kernels. */
int samaudio_op_activity(const float* wav, int rows, int64_t row_stride, int64_t samples, int step, int phases,
                         const int32_t* threshold_table /* [32769] */, const double* ref_spans /* [n_ref][2] s, or NULL */,
                         int n_ref, int metric, void* workspace, int64_t workspace_bytes, float* scores, int32_t* spans,
                         int max_spans, int32_t* span_count, int32_t* peak, samaudio_stream stream);

/* ---- CLAP log-mel front end: `rows` mono waveforms -> [rows][frames][n_mels] dB features -----
 * What `transformers.ClapFeatureExtractor(truncation="rand_trunc", padding="repeatpad")` computes for one clip, with the reference
 * ranker's int16 round trip in front (sam_audio/ranking/clap.py:50-52), as one kernel; nothing but the features is stored.  The CPU
 * statement is tests/clap_ref.py - pinned to ClapFeatureExtractor, unpinned vs laion_clap.  Per row, with n = lengths[r],
 * L = max_length, N = fft_size:
 *   1  quantise != 0: x = float(trunc(clamp(x, -1, 1) * SAMAUDIO_CLAP_INT16_SCALE)) / SAMAUDIO_CLAP_INT16_SCALE, each operation
 *      rounded to fp32 as torch does it
 *   2  n < L ("repeatpad"): y[i] = x[i % n] for i < (L / n) n, 0 behind;  n == L: y = x;  n > L: y[i] = x[offsets[r] + i], i < L
 *      (the extractor draws that offset at random; the caller decides here)
 *   3  frames = 1 + L / hop centred frames: frame f is y[f hop - N / 2 + j], j < N, reflected at both ends (y[-i] = y[i],
 *      y[L - 1 + i] = y[L - 1 - i]), times window[j] (the caller's; the extractor's is the periodic Hann window)
 *   4  X = the real DFT of the frame (a complex FFT of N / 2 points in LDS and one untangling pass), P[k] = |X[k]|^2, k <= N / 2
 *   5  mel[m] = sum_k bank[k][m] P[k] (bank [N / 2 + 1][n_mels] f32, the caller's: any of the extractor's filter banks)
 *   6  dB = 10 log10(max(mel, 1e-10)), exactly -100 at and below the floor;  out = dB * bn_scale[m] + bn_shift[m] where both are
 *      given (the audio tower's eval-mode BatchNorm2d over the mel bins, folded by the caller)
 * tables [2 N] f32 (device): window [N], then (cos, -sin)(2 pi t / N) interleaved for t < N / 2 - evaluated by the caller in
 * float64 (sam_audio_amd/clap.py logmel_tables).  lengths / offsets are HOST arrays [rows] (offsets NULL = 0; it is read for rows
 * longer than L only); consecutive rows of equal length and offset share a launch.  A frame's value does not depend on the other
 * frames, the other rows or the launch geometry. */
#define SAMAUDIO_CLAP_INT16_SCALE 32767.0f   /* laion_clap's float32_to_int16 / int16_to_float32 constant: unpinned (laion_clap is absent) */
/* 1 + max_length / hop; -1 for an argument below 1 */
int64_t samaudio_logmel_frames(int64_t max_length, int hop);
/* out [rows][frames][n_mels] f32.  Stateless, no workspace, nothing is read back.  SAMAUDIO_ERR_ARG before any launch for a null
 * wav / lengths / tables / bank / out, only one of bn_scale / bn_shift, rows / hop / n_mels < 1, fft_size not a power of two in
 * [64, 2048], max_length <= fft_size / 2 (no reflection) or >= 2^30, a length < 1 or > row_stride (rows > 1), an offset outside
 * [0, n - max_length]; SAMAUDIO_ERR_STATE in a build of the library without the kernel. */
int samaudio_op_logmel(const float* wav, int rows, int64_t row_stride, const int64_t* lengths, const int64_t* offsets,
                       int64_t max_length, int quantise, int fft_size, int hop, int n_mels, const float* tables,
                       const float* bank, const float* bn_scale, const float* bn_shift, float* out, samaudio_stream stream);

/* ---- CLAP ranker towers ---------------------------------------------------------------------
 * `transformers.ClapModel` without feature fusion: get_audio_features (the log-mel front end above with the BatchNorm folded in,
 * the HTSAT audio tower - mel-to-image patch embedding, stages of shifted-window attention blocks, patch merging - the final
 * LayerNorm, the mean over all tokens, audio_projection, L2 normalisation) and get_text_features (the RoBERTa text tower, its
 * pooler, text_projection, L2 normalisation).  fp32 only; the towers own no device memory: borrowed weights, one caller workspace.
 * Engine tensor names: sam_audio_amd/clap.py documents the mapping from ClapModel's state_dict keys. */
typedef struct {
  /* front end */
  int32_t fft_size, hop, max_length;          /* 1024, 480, 480000 */
  /* audio tower */
  int32_t spec_size, num_mel_bins;            /* 256, 64: spec_size % num_mel_bins == 0 (freq_ratio), frames <= spec_size * freq_ratio */
  int32_t patch_size, patch_stride;           /* 4, 4 */
  int32_t embed_dim;                          /* patch_embeds_hidden_size, 96; stage s is embed_dim << s wide */
  int32_t num_stages;                         /* 4 (<= 4) */
  int32_t depths[4], heads[4];                /* {2, 2, 6, 2}, {4, 8, 16, 32}: head width 24 or 32 */
  int32_t window_size;                        /* 8 (window_size^2 <= 64) */
  int32_t mlp_ratio;                          /* 4 */
  int32_t patch_norm;                         /* enable_patch_layer_norm */
  int32_t enable_fusion;                      /* must be 0: refused at create */
  float audio_ln_eps;                         /* layer_norm_eps of the blocks, 1e-5 (the patch, merge and final norms are 1e-5 as nn.LayerNorm) */
  /* text tower */
  int32_t text_vocab, text_hidden, text_heads, text_layers, text_intermediate;   /* 50265, 768, 12, 12, 3072 */
  int32_t text_max_positions, text_pad_id;    /* 514 (<= 514), 1 */
  float text_ln_eps;                          /* 1e-12 */
  int32_t projection_dim;                     /* 512 */
} samaudio_clap_config;
typedef struct samaudio_clap samaudio_clap;
int samaudio_clap_create(const samaudio_clap_config* cfg, samaudio_clap** out);
void samaudio_clap_destroy(samaudio_clap* t);
int samaudio_clap_set_tensor(samaudio_clap* t, const char* name, const void* data, int dtype, int ndim, const int64_t* shape);
/* resolves the weights; SAMAUDIO_ERR_ARG when a GEMM's K (a stage width, its MLP width, 4 x a merged width, text_hidden,
 * text_intermediate) is no multiple of 32, a resolution is no multiple of its window or odd before a merge, a head width is neither 24
 * nor 32; SAMAUDIO_ERR_WEIGHT for a missing or misshapen tensor */
int samaudio_clap_finalize(samaudio_clap* t);
/* bytes for audio_rows clips and text_rows x tokens tokens (either may be 0); the two towers share the workspace */
size_t samaudio_clap_workspace_bytes(samaudio_clap* t, int audio_rows, int text_rows, int tokens);
int samaudio_clap_set_workspace(samaudio_clap* t, void* workspace, size_t bytes);
/* out [rows][projection_dim] f32, unit norm: waveforms as samaudio_op_logmel takes them (lengths / offsets are host arrays).
 * SAMAUDIO_ERR_ARG for a clip of length < 1 (and what samaudio_op_logmel refuses), SAMAUDIO_ERR_WORKSPACE for a workspace that is
 * missing or too small */
int samaudio_clap_audio_embed(samaudio_clap* t, const float* wav, int rows, int64_t row_stride, const int64_t* lengths,
                              const int64_t* offsets, int quantise, float* out, samaudio_stream stream);
/* out [rows][projection_dim] f32, unit norm: input_ids [rows][tokens] i64 and attention_mask [rows][tokens] u8 (device).
 * SAMAUDIO_ERR_ARG for tokens + text_pad_id + 1 > text_max_positions (the position table) */
int samaudio_clap_text_embed(samaudio_clap* t, const int64_t* input_ids, const unsigned char* attention_mask, int rows, int tokens,
                             float* out, samaudio_stream stream);
/* scores [clips][candidates] = <audio [clips * candidates][dim], text [clips][dim]>: the reference's [B, cand, E] @ [B, E, 1] */
int samaudio_clap_score(const float* audio, const float* text, int clips, int candidates, int dim, float* scores,
                        samaudio_stream stream);
/* the tower's new kernels alone, for tests (csrc/kernels.h launch_clap_patch_embed / launch_swin_window_attn /
 * launch_swin_patch_merge say what they compute); SAMAUDIO_ERR_ARG for what a launcher's comment excludes */
int samaudio_op_clap_patch_embed(const float* feat, int n, int frames, int n_mels, int spec_size, int patch_size, int patch_stride,
                                 int dim, const float* w, const float* bias, const float* ln_w, const float* ln_b, float eps,
                                 float* tokens, samaudio_stream stream);
int samaudio_op_swin_window_attn(const float* qkv, const float* table, float* out, int n, int height, int width, int heads,
                                 int head_dim, int window, int shift, samaudio_stream stream);
int samaudio_op_swin_patch_merge(const float* x, const float* ln_w, const float* ln_b, float eps, float* out, int n, int height,
                                 int width, int dim, samaudio_stream stream);

/* ---- text-prompt encoder ---------------------------------------------------------
 * T5 encoder stack behind `T5TextEncoder.forward` (reference sam_audio/model/text_encoder.py:19-37:
 * `transformers.T5EncoderModel("t5-base")(input_ids, attention_mask)["last_hidden_state"]`).  Tokenisation stays with the
 * caller (the Hugging Face tokenizer, text_encoder.py:21-27); everything from the embedding lookup to the final
 * T5LayerNorm runs here.  Engine tensor names: sam_audio_amd/t5_encoder.py documents the mapping from the
 * `shared.* / encoder.*` state_dict keys. */
typedef struct {
  int32_t precision;                 /* SAMAUDIO_F32 | SAMAUDIO_BF16 (GEMM operands; the residual stream is f32) */
  int32_t vocab, d_model, d_kv;      /* 32128, 768, 64 (d_kv <= 128) */
  int32_t heads, d_ff, layers;       /* 12, 3072, 12; heads * d_kv and d_ff must be multiples of 64 */
  int32_t max_len;                   /* longest sequence the relative-position table covers (<= 512) */
  int32_t act;                       /* 6 = ReLU (t5-base), 7 = tanh-form GELU ("gelu_new"); gated variants unsupported */
  float ln_eps;                      /* 1e-6 */
} samaudio_t5_config;

typedef struct samaudio_t5 samaudio_t5;
int samaudio_t5_create(const samaudio_t5_config* cfg, samaudio_t5** out);
void samaudio_t5_destroy(samaudio_t5* t);
int samaudio_t5_set_tensor(samaudio_t5* t, const char* name, const void* data, int dtype, int ndim,
                           const int64_t* shape);
int samaudio_t5_finalize(samaudio_t5* t);
size_t samaudio_t5_workspace_bytes(samaudio_t5* t, int rows, int tokens);
int samaudio_t5_set_workspace(samaudio_t5* t, void* workspace, size_t bytes);
/* input_ids [rows, tokens] i64 (device), attention_mask [rows, tokens] u8 (1 = token, device) ->
 * last_hidden_state [rows, tokens, d_model] f32, every position (padding rows included, as transformers returns them).
 * An id outside [0, vocab) is the caller's error: the lookup clamps it. */
int samaudio_t5_encode(samaudio_t5* t, const int64_t* input_ids, const unsigned char* attention_mask, int rows, int tokens,
                       float* last_hidden_state, samaudio_stream stream);

/* ---- Judge / span-predictor text tower -------------------------------------------
 * ModernBERT encoder behind `SAMAudioJudgeModel._get_text_output` and `PEAudioFrame` (reference sam_audio/model/judge.py:48,
 * 74-88: `transformers.AutoModel.from_config(ModernBertConfig(...))`, `hidden_states[nth_text_layer]`).  Tokenisation stays
 * with the caller; everything from the embedding lookup to the requested hidden state runs here.  Engine tensor names:
 * sam_audio_amd/mbert_encoder.py documents the mapping from the `embeddings.* / layers.* / final_norm.*` state_dict keys. */
typedef struct {
  int32_t precision;                  /* SAMAUDIO_F32 | SAMAUDIO_BF16 (GEMM operands; the residual stream is f32) */
  int32_t vocab, hidden, heads;       /* 50368, 768, 12 (head dim even, <= 128) */
  int32_t intermediate, layers;       /* 1152 (Wi projects to 2x that: input | gate), 22 */
  int32_t global_every;               /* 3: layers l % 3 == 0 attend globally, the others within +-window tokens */
  int32_t window;                     /* 64 = local_attention / 2 */
  int32_t max_len;                    /* longest sequence the rotary tables cover (<= 512) */
  float ln_eps;                       /* 1e-5 */
} samaudio_mbert_config;

typedef struct samaudio_mbert samaudio_mbert;
int samaudio_mbert_create(const samaudio_mbert_config* cfg, samaudio_mbert** out);
void samaudio_mbert_destroy(samaudio_mbert* t);
int samaudio_mbert_set_tensor(samaudio_mbert* t, const char* name, const void* data, int dtype, int ndim,
                              const int64_t* shape);
int samaudio_mbert_finalize(samaudio_mbert* t);
size_t samaudio_mbert_workspace_bytes(samaudio_mbert* t, int rows, int tokens);
int samaudio_mbert_set_workspace(samaudio_mbert* t, void* workspace, size_t bytes);
/* input_ids [rows, tokens] i64, attention_mask [rows, tokens] u8 (1 = token) -> hidden [rows, tokens, hidden] f32.
 * nth_hidden_state: 0 <= n <= layers = the residual stream after n layers (0 = the normalised embeddings), NEVER passed
 * through final_norm; n < 0 = last_hidden_state (after the final LayerNorm).  The two transformers generations disagree
 * about hidden_states[layers] - 4.48 .. 4.5x (what the reference pins, pyproject.toml: transformers>=4.54, and what the
 * released Judge was trained with) append the last layer's output BEFORE final_norm, 5.x records the normalised tensor -
 * and the reference's default nth_text_layer = 22 = layers selects exactly that entry (judge.py:74-88).  The ABI is
 * explicit: n == layers is the pre-norm tensor; a caller that wants 5.x semantics passes -1 (the host classes do this
 * under SAMAudioJudgeConfig.last_text_layer_prenorm = False). */
int samaudio_mbert_encode(samaudio_mbert* t, const int64_t* input_ids, const unsigned char* attention_mask, int rows, int tokens,
                          int nth_hidden_state, float* hidden, samaudio_stream stream);

/* ---- measurement ----------------------------------------------------------------------------------- */

/* Live per-kernel timing for bench.py's roofline leg (the reference has no counterpart: it publishes no
 * throughput numbers).  Between begin and end every GEMM launch on the hot path is
 * bracketed by a hipEvent pair recorded on the launch stream; end synchronises and returns, per GEMM tile
 * variant, the number of launches, the summed ALGORITHMIC flops (2*M*N*K of the contraction, zero padding
 * of K excluded) and the summed event time in ms. */
typedef struct {
  char name[64];
  int64_t launches;
  double flops; /* algorithmic flops of the launches (2*M*N*K for a contraction; 0 for pure streaming kernels) */
  double bytes; /* algorithmic bytes of the launches: every operand, output and residual element counted once */
  double ms;
} samaudio_kernel_stat;
int samaudio_profile_begin(samaudio_ctx* ctx);
/* SAMAUDIO_OPT_SENTINEL: synchronises `stream`, copies out absmax[SAMAUDIO_SENTINEL_SLOTS] / nonfinite[SAMAUDIO_SENTINEL_SLOTS]
 * (counts as doubles) accumulated since the last read, and resets them. */
int samaudio_sentinel_read(samaudio_ctx* ctx, float* absmax, double* nonfinite, samaudio_stream stream);
/* Test hook: force the GEMM kernel variant (-1 automatic; otherwise an id of csrc/kernels.h `enum GemmVariant`, whose numbers are
 * kept stable: 0..2 the 128-row tiles of gemm.hip; 22 = gemm8 256x256 8-phase, 27 = gemm8s 128x128; 25 / 26 / 28 / 29 / 32 / 33 /
 * 34 = the 32x32x16-family tiles, 35 = conv7h; csrc/kernels.h kGemmVariantTable has the names).  A launch the forced kernel does
 * not cover falls back to gemm.hip's tiles - except launches on K-tile-major weights or with the split-form output, which exist in
 * the 8-phase family only: forcing anything outside that family on them is refused with SAMAUDIO_ERR_ARG and that reason (a
 * model's own launches never leave the family). */
void samaudio_debug_force_gemm_variant(int variant);
/* Test hooks (csrc/kernels.h `enum DebugFlag` names and documents every one, sam_audio_amd/hip.py mirrors the names; the numbers
 * are kept stable; 0 = shipped behaviour): 11 = k7 convolutions as implicit GEMMs, 16 = DAC residual
 * units as two launches, 18 = fuse residual units whatever the launch size, 19 = residual-unit kernel form (1 / 3 = weight-
 * stationary, 2 = ring), 21 = gemm8s always in its plain double-buffered form, 24 = epilogue form of the 8-phase family (1 = the
 * general one for every launch, 2 / 3 = one lean form for every eligible launch), 26 = 1: one workgroup per tile (shipped:
 * persistent above 256 tiles). */
void samaudio_debug_set_flag(int flag, int value);
/* Test aid: leave the LDS of every CU filled with NaN bit patterns (LDS is not cleared between kernels), so that a
 * kernel consuming LDS it never wrote fails deterministically. */
int samaudio_debug_poison_lds(samaudio_stream stream);
int samaudio_profile_end(samaudio_ctx* ctx, samaudio_kernel_stat* out, int capacity, int* count);

/* ---- per-kernel hooks (parity tests; each is one kernel of the path above) -------------------------- */

/* C[b] = epilogue(A(b) @ W^T): generalised GEMM / implicit conv, see sam_audio_amd/csrc/common.h GemmParams.
 * `params` points to a HOST copy of sa::GemmParams (size checked against params_bytes). */
int samaudio_op_gemm(const void* params_host, size_t params_bytes, int precision, samaudio_stream stream);
/* One DAC-VAE convolution the way an fp32 context with SAMAUDIO_OPT_X3_CLASSES bit CODEC runs it (csrc/host.h codec_x3_* - the
 * functions the engine itself launches by).  `params_host`: the convolution's plain fp32 GemmParams, as for samaudio_op_gemm (fp32 A,
 * fp32 outputs, W = the fp32 weight).  `w_twin`: the weight's registered twin - SAMAUDIO_CODEC_TWIN_FLY: "<name>.fly" (weights.py
 * fly16_weight), SAMAUDIO_CODEC_TWIN_X3: "<name>.x3" with Cin-blocks of `cin` channels (weights.py convert_codec_x3), _NONE: no twin.
 * With an x3 twin, `scratch` (>= 3 x 2 bytes per element of the halo buffers the launch reads) and a launch that qualifies, it runs
 * as split3 + ONE 16-bit launch over K' = 3K + the elementwise activation pass; otherwise on operands split in registers.  `path`
 * (may be null) receives the SAMAUDIO_CODEC_PATH_* taken. */
enum { SAMAUDIO_CODEC_TWIN_NONE = 0, SAMAUDIO_CODEC_TWIN_FLY = 1, SAMAUDIO_CODEC_TWIN_X3 = 2 };
enum { SAMAUDIO_CODEC_PATH_FLY = 0, SAMAUDIO_CODEC_PATH_X3_BLOCK = 1, SAMAUDIO_CODEC_PATH_X3 = 2 };
int samaudio_op_codec_conv(const void* params_host, size_t params_bytes, const void* w_twin, int twin_kind, int cin, void* scratch,
                           size_t scratch_bytes, int* path, samaudio_stream stream);
/* One DAC residual unit as ONE kernel: the k7 convolution `conv7_params` and the k1 convolution `conv1_params` that reads
 * its output (two host GemmParams as for samaudio_op_gemm, 16-bit operands only).  The intermediate activation
 * (conv7_params.out_act == conv1_params.A) is never written; conv1_params.out_act must not be conv7_params.A.  Bitwise
 * equal to the two samaudio_op_gemm launches; ERR_ARG when the pair is not one the fused kernel covers. */
int samaudio_op_resunit(const void* conv7_params_host, const void* conv1_params_host, size_t params_bytes,
                        samaudio_stream stream);
/* ---- the norm kernels (tests/test_norm_kernels_gpu.py).  Each hook refuses, as SAMAUDIO_ERR_ARG with a message naming the argument,
 * what its kernels assume - null required pointers; rows / batch / frames / dim (channels) <= 0, halo < 0, rows_per_batch <= 0;
 * dim % 4; fp32 base pointers off 16 bytes (a 16-bit output: 8; partials_f64: 8) - and launches nothing then. */
/* out[r] = rms_norm(x[r]) * w, and with a time vector ... * (1 + scale_tab + tvec[r / rows_per_batch][scale_off ..]) + shift_tab +
 * tvec[..][shift_off ..]: x [rows, dim] f32, out [rows, dim] in `precision`'s storage type, tvec rows tvec_ld floats apart (0: one
 * row for all).  shift_tab, scale_tab and tvec are given together or all null (plain RMSNorm); tvec_ld, shift_off, scale_off % 4. */
int samaudio_op_rmsnorm_mod(const float* x, const float* w, const float* shift_tab, const float* scale_tab,
                            const float* tvec, int64_t tvec_ld, int shift_off, int scale_off, void* out,
                            int precision, int rows, int dim, int rows_per_batch, float eps, samaudio_stream stream);
/* GroupNorm(1 group) + SiLU, channels-last: x [batch, frames, channels] f32, statistics per item over all its entries,
 * partials_f64: batch*64*2 doubles of scratch (every one written before it is read), out [batch][halo + frames + halo][channels]
 * (halo rows untouched) */
int samaudio_op_groupnorm_silu(const float* x, const float* w, const float* b, void* partials_f64, void* out,
                               int precision, int batch, int frames, int channels, int halo, float eps,
                               samaudio_stream stream);
int samaudio_op_qkv_prep(const void* qkv, const float* q_w, const float* k_w, const float* rope_cos,
                         const float* rope_sin, void* q, void* k, void* vt, int precision, int batch, int frames,
                         int frames_padded, int heads, float eps, samaudio_stream stream);
int samaudio_op_self_attention(const void* q, const void* k, const void* vt, const uint8_t* key_mask, void* out,
                               int precision, int batch, int frames, int frames_padded, int heads,
                               samaudio_stream stream);
int samaudio_op_cross_attention(const void* q, const float* q_w, void* kv, const float* k_w, const uint8_t* mask,
                                void* out, int precision, int batch, int frames, int text_len, int heads, float eps,
                                samaudio_stream stream);
/* U^T[b][n][h*ltp + j] = sum_d wo[n][h*128+d] * V[b][j][h*128+d] (bf16; V = columns [D, 2D) of kv rows b*text_len+j):
 * the per-batch operand of the folded cross-attention output projection. */
int samaudio_op_cross_attn_fold(const void* wo, const void* kv, int64_t kv_ld, void* ut, int kp, int batch, int text_len,
                                int ltp, int heads, samaudio_stream stream);
/* acc[r] += tanh(gate[0]) * (LayerNorm(x[r]) * w + b), in place: x, acc [rows, dim] f32, gate one float on the device */
int samaudio_op_layernorm_accum(const float* x, const float* w, const float* b, const float* gate, float* acc,
                                int rows, int dim, float eps, samaudio_stream stream);
/* masked GroupNorm(1) + SiLU of the PE-AV patch embedder: x [batch, frames, channels] f32, mask [batch, frames] u8,
 * partials_f64: batch*64*3 doubles of scratch, out [batch][halo + frames + halo][channels] (halo rows untouched) */
int samaudio_op_masked_groupnorm_silu(const float* x, const float* w, const float* b, const uint8_t* mask,
                                      void* partials_f64, void* out, int precision, int batch, int frames,
                                      int channels, int halo, float eps, samaudio_stream stream);
/* the same with the output as a compensated GEMM operand (SAMAUDIO_OPT_X3_CLASSES): out3 [batch][halo + frames + halo][3 channels] in
 * the library's 16-bit format, a valid frame = [lo | hi | hi] of the fp32 kernel's value, a masked frame zeros, halo rows untouched */
int samaudio_op_masked_groupnorm_silu_split3(const float* x, const float* w, const float* b, const uint8_t* mask,
                                             void* partials_f64, void* out3, int batch, int frames, int channels, int halo,
                                             float eps, samaudio_stream stream);
/* LayerNorm(x[r]) * w + b: x rows x_ld floats apart (x_ld % 4, x_ld >= dim), out_f32 [rows, dim] and / or out_act [rows, dim] in
 * `precision`'s storage type (the fp32 value rounded to nearest even); either may be null, not both */
int samaudio_op_layernorm_rows(const float* x, int64_t x_ld, const float* w, const float* b, float* out_f32,
                               void* out_act, int precision, int64_t rows, int dim, float eps, samaudio_stream stream);
/* the same with the output as a compensated GEMM operand (SAMAUDIO_OPT_X3_CLASSES; the PE-Core vision tower's LayerNorms in front of
 * q|k|v, c_fc and pool.wkv): out3 [rows, 3 dim] in the library's 16-bit format = [lo | hi | hi] of the fp32 value, bitwise what
 * samaudio_op_layernorm_rows (fp32 output) followed by samaudio_op_split3 writes.  dim % 8 == 0, dim <= 2048.  SAMAUDIO_ERR_STATE in a
 * build of the library without the kernel. */
int samaudio_op_layernorm_rows_split3(const float* x, int64_t x_ld, const float* w, const float* b, void* out3, int64_t rows,
                                      int dim, float eps, samaudio_stream stream);
/* SAMAUDIO_OPT_X3_CLASSES: the activation operand of a compensated GEMM - x [rows, k] f32 (row stride x_ld) -> out [rows, 3k]
 * in the library's 16-bit format = [lo | hi | hi] per row, hi = rn16(x) (clamped to the largest finite value), lo = rn16(x - hi) */
int samaudio_op_split3(const float* x, int64_t x_ld, void* out, int64_t rows, int k, samaudio_stream stream);

/* ---- the kernels a DiT layer launches, one hook each (tests/test_layer_kernels_gpu.py) ------------------- */

/* RMSNorm + modulate operands of one evaluation: for norm n < n_norms (HOST arrays of device pointers / offsets) and time value t,
 * gs[n][t] = [g | s] (2 * dim floats), g = w[n] * (1 + scale_tab[n] + tvec[t * tvec_ld + scale_off[n] + :]),
 * s = shift_tab[n] + tvec[t * tvec_ld + shift_off[n] + :] */
int samaudio_op_mod_tables(const float* const* w, const float* const* shift_tab, const float* const* scale_tab,
                           const int* shift_off, const int* scale_off, int n_norms, const float* tvec, int64_t tvec_ld,
                           int n_time, float* gs, int dim, samaudio_stream stream);
/* out[m, :] = rmsnorm(x[m, :]) * g + s with [g | s] = gs + (m / rows_per_batch) * gs_ld (one norm's slice of the table above;
 * gs_ld = 0: one time value for every row); dim <= 3072.  form 0: out [rows, dim] in the activation type of `precision`,
 * 1: in the alt 16-bit format (16-bit precision only), 2: out [rows, 3 * dim] 16-bit = [lo | hi | hi] (fp32 precision only) */
int samaudio_op_rmsnorm_gs(const float* x, const float* gs, int64_t gs_ld, void* out, int precision, int form, int rows,
                           int dim, int rows_per_batch, float eps, samaudio_stream stream);
/* samaudio_op_qkv_prep with head_dim 64 | 128 (rope tables [frames, head_dim / 2]).  form 0: the kernel of `precision`,
 * 1: the fp32 fast path of the compensated mode (fp32 tensors, head_dim 128 only) */
int samaudio_op_qkv_prep_hd(const void* qkv, const float* q_w, const float* k_w, const float* rope_cos,
                            const float* rope_sin, void* q, void* k, void* vt, int precision, int form, int batch,
                            int frames, int frames_padded, int heads, int head_dim, float eps, samaudio_stream stream);
/* samaudio_op_self_attention with head_dim 64 | 128; precision 2 = the compensated kernel (fp32 tensors).  form 0: out
 * [batch * frames, heads * head_dim] in the activation type, 1: the same in the alt 16-bit format (precision 1 only),
 * 2: out [batch * frames, 3 * heads * head_dim] 16-bit = [lo | hi | hi] (precision 2 only) */
int samaudio_op_self_attention_hd(const void* q, const void* k, const void* vt, const uint8_t* key_mask, void* out,
                                  int precision, int form, int batch, int frames, int frames_padded, int heads,
                                  int head_dim, samaudio_stream stream);
/* samaudio_op_cross_attention with head_dim 64 | 128 and kv rows of stride kv_ld >= 2 * heads * head_dim elements ((k | v) in
 * columns [0, 2 D) of the pointer handed in; k is normalised in place first, at that width) */
int samaudio_op_cross_attention_hd(const void* q, const float* q_w, void* kv, int64_t kv_ld, const float* k_w,
                                   const uint8_t* mask, void* out, int precision, int batch, int frames, int text_len,
                                   int heads, int head_dim, float eps, samaudio_stream stream);
/* folded cross-attention, 16-bit: p[m][h * ltp + j] = softmax probability of token j < ltp (0 for masked tokens and for
 * j >= text_len; columns >= heads * ltp of the ldp-wide row are not written); q raw (q-norm applied here), k already normalised */
int samaudio_op_cross_attn_probs(const void* q, const float* q_w, const void* kv, int64_t kv_ld, const uint8_t* mask, void* p,
                                 int ldp, int batch, int frames, int text_len, int ltp, int heads, float eps,
                                 samaudio_stream stream);
/* the same on fp32 tensors as the compensated operand p3 [rows, 3 * kp] 16-bit = [P_lo | P_hi | P_hi] */
int samaudio_op_cross_attn_probs3(const float* q, const float* q_w, const float* kv, int64_t kv_ld, const uint8_t* mask, void* p3,
                                  int kp, int batch, int frames, int text_len, int ltp, int heads, float eps,
                                  samaudio_stream stream);
/* samaudio_op_cross_attn_fold on fp32 tensors (one layer): ut3 [batch][D][3 * kp] 16-bit = [U_hi | U_lo | U_hi] */
int samaudio_op_cross_attn_fold3(const float* wo, const float* kv, int64_t kv_ld, void* ut3, int kp, int batch, int text_len,
                                 int ltp, int heads, samaudio_stream stream);

/* ---- the kernels only the towers launch, one hook each (tests/test_tower_kernels_gpu.py) ------------------
 * T5 prompt encoder, ModernBERT and CLAP text towers (t5_kernels.hip), PE-Core vision tower (vit_kernels.hip), Judge and span
 * predictor (peav_kernels.hip).  Each hook refuses with SAMAUDIO_ERR_ARG, before any launch, what its kernel cannot do - the limits the
 * towers' host code otherwise guarantees - and adds no arithmetic.  `precision` is the storage type of the tensors marked "act"
 * (SAMAUDIO_F32 | SAMAUDIO_BF16 = the library's 16-bit format).  SAMAUDIO_ERR_STATE ("not in this build of the library") in a build
 * without t5_kernels.hip / vit_kernels.hip (the CPU emulation of the launchers). */

/* t5_attention_kernel: out [batch * tokens, heads * head_dim] act = softmax(scale * q k^T + bias[h][k - q] + key mask) v on q|k|v rows
 * qkv [batch * tokens, 3 * heads * head_dim] act.  mask [batch, tokens] bytes (non-zero = key allowed); bias [heads, 2 * max_len - 1]
 * f32 with the distance k - q at column k - q + max_len - 1, or NULL; window > 0: only keys with |k - q| <= window.  The softmax runs
 * over the allowed keys; a row without one attends uniformly over all `tokens` keys; every query row is written, masked ones too.
 * Refused: tokens outside [1, 512], head_dim outside [1, 128], a bias with max_len < tokens, null qkv / mask / out. */
int samaudio_op_tower_attention(const void* qkv, const uint8_t* mask, const float* bias, void* out, int precision, int batch,
                                int tokens, int heads, int head_dim, int max_len, float scale, int window, samaudio_stream stream);
/* mbert_rope_kernel, in place: x' = x * cos + rotate_half(x) * sin on the q and k segments of qkv [rows, 3 * heads * head_dim] act,
 * row m at position m % tokens of rope_cos / rope_sin [>= tokens, head_dim] f32; the v segment is not touched.  Refused: odd head_dim. */
int samaudio_op_mbert_rope(void* qkv, const float* rope_cos, const float* rope_sin, int precision, int64_t rows, int tokens, int heads,
                           int head_dim, samaudio_stream stream);
/* geglu_kernel: out [rows, features] act = gelu(x[:, :features]) * x[:, features:] (erf form) of x [rows, 2 * features] act */
int samaudio_op_geglu(const void* x, void* out, int precision, int64_t rows, int features, samaudio_stream stream);
/* rope2d_split_kernel (fp32) / rope2d_split_bf16_kernel (16-bit): q|k|v rows qkv [n * tokens, 3 * heads * head_dim] act -> q, k
 * [n, heads, tokens_padded, head_dim] with (x0, x1) -> (x0 c - x1 s, x0 s + x1 c) on adjacent pairs, c / s = rope_cos / rope_sin
 * [tokens, head_dim / 2] f32 (both NULL: a copy), and vt [n, heads, head_dim, tokens_padded] = V^T; rows / columns tokens ..
 * tokens_padded are written as zeros.  Refused: head_dim other than 64 | 128, tokens_padded % 64, tokens_padded < tokens, one table
 * without the other, 16-bit: a pointer that is not aligned to 16 bytes. */
int samaudio_op_rope2d_split(const void* qkv, const float* rope_cos, const float* rope_sin, void* q, void* k, void* vt, int precision,
                             int n, int tokens, int tokens_padded, int heads, int head_dim, samaudio_stream stream);
/* pool_attention_kernel: out [n, heads * head_dim] act = softmax_t(q_h . k[f, t, h] * head_dim^-0.5) . v[f, t, h] for one query
 * q [heads * head_dim] f32 over kv [n * tokens, 2 * heads * head_dim] act = (k | v).  Refused: head_dim other than 64 | 128, tokens < 1. */
int samaudio_op_pool_attention(const float* q, const void* kv, void* out, int precision, int n, int tokens, int heads, int head_dim,
                               samaudio_stream stream);
/* l2_normalize_kernel, in place: x[r, :] /= max(||x[r, :]||, 1e-12) on x [rows, dim] f32 */
int samaudio_op_l2_normalize(float* x, int rows, int dim, samaudio_stream stream);
/* token_mean_kernel: mean over the `tokens` rows of each item of x [n * tokens, x_ld] f32 (columns [0, dim)) -> out_f32 [n, dim] f32
 * and / or out_act [n, dim] act (the same fp32 value, rounded).  Refused: both outputs NULL, x_ld < dim. */
int samaudio_op_token_mean(const float* x, int64_t x_ld, float* out_f32, void* out_act, int precision, int n, int tokens, int dim,
                           samaudio_stream stream);
/* peav_cls_mask_kernel: h [batch, frames + 1, dim] f32: row 0 of every item = cls [dim], the other rows are not touched;
 * mask_s [batch, frames + 1] bytes: mask_s[b][0] = pad[b][0] != 0, mask_s[b][1 + t] = pad[b][t] != 0 (pad [batch, frames] bytes; NULL:
 * all 1).  Refused: dim % 4, h or cls not aligned to 16 bytes. */
int samaudio_op_peav_cls_mask(float* h, const float* cls, const uint8_t* pad, uint8_t* mask_s, int batch, int frames, int dim,
                              samaudio_stream stream);
/* judge_pool_head_kernel: out [batch, 4] f32 = (mean over the frames t with mask_s[b][1 + t] != 0 of hidden[b][1 + t][:]) . head_w[j][:]
 * * std[j] + mean[j]; hidden [batch, frames + 1, dim] f32 (row 0, the class token, and mask_s[b][0] are not read), head_w [4, dim];
 * an item without a valid frame yields mean.  Refused: dim > 4096. */
int samaudio_op_judge_pool_head(const float* hidden, const uint8_t* mask_s, const float* head_w, const float* mean, const float* std_,
                                float* out, int batch, int frames, int dim, samaudio_stream stream);
/* frame_logits_kernel: out [batch, frames] f32 = <audio[a_off + b * a_bstride + t * embed_dim + :], text[b][:]> * scale[0] + bias[0]
 * (scale, bias: device scalars).  Refused: embed_dim % 4, a_off % 4, a_bstride % 4, audio or text not aligned to 16 bytes. */
int samaudio_op_frame_logits(const float* audio, int64_t a_bstride, int64_t a_off, const float* text, const float* scale,
                             const float* bias, float* out, int batch, int frames, int embed_dim, samaudio_stream stream);

/* ---- the glue kernels between those, one hook each (tests/test_glue_kernels_gpu.py) ------------------------
 * kernels.hip, peav_kernels.hip, t5_kernels.hip, clap_kernels.hip.  Each hook refuses with SAMAUDIO_ERR_ARG, before any launch, null
 * pointers, sizes < 1 and what its kernel cannot do, then calls the launcher the engine and the towers call; no arithmetic here.
 * `precision` as above (the storage type of the tensors marked "act").  SAMAUDIO_ERR_STATE ("not in this build of the library") where
 * the launcher is missing (the CPU emulation of the launchers: ode_stage, embed_rows, clap_text_embed, sentinel). */

/* time_features_kernel: temb [n_time, freq_dim] act = (cos | sin)(t[j] * freqs[i]), i < freq_dim / 2, and tsin [n_time, dim] f32 =
 * (cos | sin)(t[j] * inv_freq[i]), i < dim / 2; t, freqs [freq_dim / 2], inv_freq [dim / 2] f32.  Refused: odd freq_dim / dim. */
int samaudio_op_time_features(const float* t, int n_time, const float* freqs, int freq_dim, const float* inv_freq, int dim, void* temb,
                              float* tsin, int precision, samaudio_stream stream);
/* add_rowvec_kernel: out [rows, dim] act = x [rows, dim] f32 + vec[(r / rows_per_batch) * vec_ld + :] (vec_ld = 0: one vector for
 * every row).  Refused: dim % 4, vec_ld % 4, x or vec not aligned to 16 bytes, out not aligned to 16 (f32) / 8 (16-bit) bytes. */
int samaudio_op_add_rowvec(const float* x, const float* vec, int64_t vec_ld, void* out, int precision, int rows, int dim,
                           int rows_per_batch, samaudio_stream stream);
/* headnorm_layers_kernel, in place: per (row, layer, head) RMSNorm over head_dim of the K half of kv_all [rows, layers * 2 * heads *
 * head_dim] act (layer l's block = (k | v), the v half is not touched), times w_all[l][:] (w_all [layers, head_dim] f32).
 * Refused: head_dim other than 64 | 128, kv_all not aligned to 8 (f32) / 4 (16-bit) bytes. */
int samaudio_op_headnorm_layers(void* kv_all, const float* w_all, int precision, int rows, int layers, int heads, int head_dim,
                                float eps, samaudio_stream stream);
/* to_act_kernel: out[b][halo + t][c] act = c < c_in ? in[b * in_bstride + in_col0 + t * in_ld + c] : 0 for t < frames, c < c_out
 * (in f32; item b of out at b * out_bstride elements, 0 = dense (frames + 2 halo) * c_out; halo rows are not touched; the cast rounds
 * to nearest even).  Refused: c_in > c_out, negative strides / offsets / halo. */
int samaudio_op_to_act(const float* in, int64_t in_bstride, int64_t in_ld, int in_col0, void* out, int64_t out_bstride, int precision,
                       int batch, int64_t frames, int c_in, int c_out, int halo, samaudio_stream stream);
/* zero_halo_kernel: rows [0, halo) and [halo + frames, frames + 2 halo) of every item of buf [batch][frames + 2 halo][channels] act
 * = +0; the other rows are not touched.  Refused: halo < 1. */
int samaudio_op_zero_halo(void* buf, int precision, int batch, int64_t frames, int channels, int halo, samaudio_stream stream);
/* anchor_gather_kernel: out [batch * frames, embed_dim] act = emb[ids[b][align[b][t]]][:] (emb [vocab, embed_dim] f32, ids [batch,
 * n_ids] i64, align [batch, frames] i64); a slot outside [0, n_ids) and a token outside [0, vocab) are clamped into range. */
int samaudio_op_anchor_gather(const float* emb, const int64_t* ids, int n_ids, const int64_t* align, void* out, int precision,
                              int batch, int frames, int embed_dim, int vocab, samaudio_stream stream);
/* set_floats_kernel: dst[0 .. n) (device) = host_values[0 .. n) (HOST), handed over as kernel arguments, 64 per launch */
int samaudio_op_set_floats(float* dst, const float* host_values, int n, samaudio_stream stream);
/* noise_rows_kernel: the seeded start state of SAMAudio.separate(seed=...) (tests/noise_ref.py is the
 * statement, this build's own: pinned to Random123's Philox4x32-10 known answers and to the float64 statement, unpinned vs torch's
 * randn).  out [clips * candidates, frames, channels] f32 contiguous, row b * candidates + c = candidate c of clip b.  The value at
 * (seed, clip id, candidate, frame t, channel ch): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (t * channels / 4 + ch / 4, candidate, id & 0xffffffff, id >> 32) yields x0..x3 for channels 4q..4q+3; (x0, x1) and (x2, x3) each
 * give r = sqrt(-2 ln(((xa >> 8) + 1) 2^-24)), th = 2 pi (xb >> 8) 2^-24, (r cos th, r sin th), |z| <= sqrt(48 ln 2).  Nothing else
 * enters: not frames, clips, candidates or the place in the batch.  clip_ids_host: HOST array [clips] of ids in [0, 2^63), handed to
 * the kernel as kernel arguments, 64 clips per launch: no upload, no synchronisation.  SAMAUDIO_ERR_ARG before any launch: null out /
 * clip_ids_host, out not aligned to 16 bytes, clips / candidates / frames < 1, channels < 4 or channels % 4 != 0,
 * frames * channels / 4 > 2^32 (counter word 0), a negative clip id.  SAMAUDIO_ERR_STATE ("not available in this build") where the
 * launcher is missing (the CPU emulation of the launchers). */
int samaudio_op_noise(float* out, int clips, int candidates, int frames, int channels, uint64_t seed, const int64_t* clip_ids_host,
                      samaudio_stream stream);
/* ode_stage_kernel: out[i] = y0[i] + scale * sum_{j < n_src} coef[j] * k[j][i] for i < n, f32; k, coef: HOST arrays of FOUR device
 * pointers / floats, of which the kernel reads the first n_src (the rest are handed to it as they are and never used: the engine
 * leaves out the sources whose tableau coefficient is 0); out may be y0.  Refused: n_src outside [1, 4], n % 4, a pointer in use
 * that is not aligned to 16 bytes. */
int samaudio_op_ode_stage(const float* y0, const float* const* k, const float* coef, int n_src, float scale, float* out, int64_t n,
                          samaudio_stream stream);
/* The kernels of samaudio_ode_solve_adaptive (kernels.hip; tests/test_ode_adaptive_gpu.py).  ctl [rows] is the per-row control block,
 * 16 words of 4 bytes each: f32 t, h (the trial step in flight), t_new, h_abs, h_prev, err, d1, h0; i32 status (SAMAUDIO_ODE_ROW_*),
 * accepted, rejected, step_rejected, accepted_now, n_valid (elements in the row's norms); two spare.  k, coef: HOST arrays of SEVEN
 * device pointers / floats of which the first n_src are read.  All device pointers aligned to 16 bytes, row_elems % 4 == 0.
 * ode_stage_rows_kernel: out[r, i] = y[r, i] + ctl[r].h * sum_j coef[j] k[j][r, i] for running rows; a row whose status is not RUNNING
 *   is copied through without its K being read.  out may be y, never a k. */
int samaudio_op_ode_stage_rows(const float* y, const float* const* k, const float* coef, int n_src, const void* ctl, float* out,
                               int rows, int64_t row_elems, samaudio_stream stream);
/* ode_error_kernel: partials [rows, chunks] f32, chunks = ceil(frames * channels / 4096): partials[r, c] = the sum over the valid
 *   elements of [4096 c, 4096 (c + 1)) of row r of (m sum_j coef[j] k[j] / (atol + rtol max(|y|, |ynew|)))^2, m = ctl[r].h if use_h else
 *   1, ynew null: |y| alone; lane-ordered adds and a fixed tree, no atomics; 0 for rows that are not running.  mask [rows, frames] u8
 *   (null: every frame valid). */
int samaudio_op_ode_error(const float* y, const float* ynew, const float* const* k, const float* coef, int n_src, const void* ctl,
                          const uint8_t* mask, float rtol, float atol, int use_h, float* partials, int rows, int frames, int channels,
                          samaudio_stream stream);
/* ode_control_kernel, one lane per row; mode 0 reset (t = t0, counters 0, n_valid from the mask; first_step > 0: the first trial),
 *   1 / 2 the two halves of the initial-step rule (1 reads partials = d0 and partials_b = d1, 2 reads partials = d2 h0), 3 the
 *   accept / reject decision on partials and the next trial.  times [stages + 1, rows] f32: the next trial's t + c_i h;
 *   *active (device i32) = rows running afterwards. */
int samaudio_op_ode_control(void* ctl, int mode, int method, float t0, float t1, const samaudio_ode_adaptive* opt, const float* partials,
                            const float* partials_b, int chunks, const uint8_t* mask, int frames, int channels, float* times,
                            int32_t* active, int rows, samaudio_stream stream);
/* ode_control_groups_kernel, one lane per group of rows (samaudio_set_window_groups): samaudio_op_ode_control's arguments, then
 *   groups [n_groups, 3] device i32 = first row, row count, row stride.  A group's sum = its rows' partials added in window order,
 *   chunk order within a row, in one f32 accumulator; n_valid = the masked frames of all its rows * channels; the decision is
 *   ode_control_kernel's, and every row of the group ends with the same 64 control bytes and time-table column.  Row indices outside
 *   [0, rows) are skipped.  groups NULL (n_groups == rows): every row is its own group, bit for bit samaudio_op_ode_control.
 *   *active = rows of groups running afterwards.  More than 256 groups: lanes loop. */
int samaudio_op_ode_control_groups(void* ctl, int mode, int method, float t0, float t1, const samaudio_ode_adaptive* opt,
                                   const float* partials, const float* partials_b, int chunks, const uint8_t* mask, int frames,
                                   int channels, float* times, int32_t* active, int rows, const int32_t* groups, int n_groups,
                                   samaudio_stream stream);
/* ode_commit_kernel: rows with accepted_now: y <- ynew, k_first <- k_last */
int samaudio_op_ode_commit(float* y, const float* ynew, float* k_first, const float* k_last, const void* ctl, int rows,
                           int64_t row_elems, samaudio_stream stream);
/* repeat_rows_u8_kernel: dst [rows * rep, width] bytes, dst[b * rep + c][:] = src[b][:] */
int samaudio_op_repeat_rows(const uint8_t* src, uint8_t* dst, int rows, int rep, int width, samaudio_stream stream);
/* repeat_items_f32_kernel: the same for items of `elems` f32 values.  Refused: elems % 4, src or dst not aligned to 16 bytes. */
int samaudio_op_repeat_items(const float* src, float* dst, int items, int rep, int64_t elems, samaudio_stream stream);
/* t5_embed_kernel (T5 and ModernBERT towers): out [rows, dim] f32 = table[ids[m]][:] (table [vocab, dim] f32, ids i64; an id outside
 * [0, vocab) is clamped into range).  Refused: dim % 4, table or out not aligned to 16 bytes. */
int samaudio_op_embed_rows(const int64_t* ids, const float* table, float* out, int64_t rows, int dim, int vocab,
                           samaudio_stream stream);
/* clap_text_embed_kernel: out [rows, tokens, dim] f32 = word[ids] + pos[position] + type[0], position = pad_id + (number of ids !=
 * pad_id in the row up to and including the token) for an id != pad_id, pad_id otherwise (transformers'
 * create_position_ids_from_input_ids); word [vocab, dim], pos [max_positions, dim], type [>= 1, dim] f32; ids outside [0, vocab) are
 * clamped.  Refused: tokens > 1024, max_positions < pad_id + tokens + 1, pad_id < 0. */
int samaudio_op_clap_text_embed(const int64_t* ids, const float* word, const float* pos, const float* type, float* out, int rows,
                                int tokens, int dim, int vocab, int pad_id, int max_positions, samaudio_stream stream);
/* sentinel_scan_kernel + sentinel_fold_kernel (SAMAUDIO_OPT_SENTINEL): scans x [rows, cols] with row pitch ld >= cols elements (the
 * pitch gap is not read) and folds into the caller's slot: slot[0] = max(slot[0], largest finite |x|), slot[1] += number of NaN and
 * +-Inf elements - every finite value counts as finite, the largest ones of bfloat16 and fp32 included.  format 0: f32, 1: the
 * library's 16-bit format, 2: the alt 16-bit format (bfloat16).  scratch: 2 * 256 floats, written by the launch (as many partials as
 * it has workgroups).  Refused: format outside 0..2, ld < cols. */
int samaudio_op_sentinel(const void* x, int format, int64_t rows, int cols, int64_t ld, float* scratch, float* slot,
                         samaudio_stream stream);
/* hash_items_kernel (SAMAUDIO_TRACE_HASH): out[b] u64 = sum_i (x[b][i] ^ (u32)(i * 0x9E3779B1)) * (2 i + 1) mod 2^64 over the
 * `words` u32 words of item b */
int samaudio_op_hash_items(const uint32_t* x, int64_t words, int items, uint64_t* out, samaudio_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SAMAUDIO_H_ */
