// Host-side orchestration of the reranking / span-prediction rows: the PE-AV
// transformer (used twice by the Judge and once by PE-A-Frame), the Judge's glue (reference
// sam_audio/model/judge.py:90-132) and the PE-A-Frame frame logits.  Like Engine, these classes own no device
// memory: weights are borrowed, scratch is one caller-provided workspace.
#pragma once
#include "host.h"

namespace sa {

// One PE-AV transformer: input projection -> [class token ; frames] -> ResNet block with masked GroupNorm ->
// n_layers x (RMSNorm, qk-norm RoPE attention, RMSNorm, SwiGLU) -> RMSNorm -> output projection.
class PeavEncoder {
 public:
  PeavEncoder(const samaudio_peav_dims& d, bool bf16, std::string prefix);
  // SAMAUDIO_OPT_X3_CLASSES of an fp32 context (mask of SAMAUDIO_CLS_X3_TOWER bits; before finalize): the switched classes multiply
  // compensated 16-bit operands - QKV / WO / W13 / W2 the four GEMMs of every layer, WO also the output projection out.w, PATCH the two
  // k3 convolutions of the ResNet block (per-tap split, plain walk), SAMAUDIO_X3_ATTENTION the self-attention.  0 = the fp32 path.
  void set_x3(int mask) { x3_ = bf16_ ? 0 : mask; ready_ = false; }
  bool x3(int cls) const { return (x3_ & cls) != 0; }
  Status finalize(const Registry& reg);
  void plan(Bump& b, int rows, int frames, bool assign);
  // x_act [rows, frames, in_dim] GEMM-operand dtype; pad_mask [rows, frames] u8 (1 = valid) or null.
  Status forward(const void* x_act, const unsigned char* pad_mask, int rows, int frames, hipStream_t st);
  // results of the last forward: [rows][frames + 1][dim], row 0 of each item = class token (pooler_output)
  const float* out_f32() const { return w_.out; }
  const void* out_act() const { return x3(SAMAUDIO_CLS_WO) ? (const void*)w_.out : w_.out_act; }   // (x3 out.w: one fp32 output)
  const unsigned char* seq_mask() const { return w_.mask_s; }  // [rows][frames + 1]
  // x3 contexts: the D-wide split scratch [rows * (frames + 1), 3 dim] 16-bit - free between two forwards (the Judge splits the
  // hidden states into it for cat_audio_proj)
  void* x3_scratch() const { return w_.x3a; }
  size_t x3_scratch_bytes() const { return w_.x3a_bytes; }
  // One launch on the weight `w`: `p` = the context's plain launch, run as it is on w.w - or, class `cls` switched to compensated
  // operands, as ONE 16-bit launch on w.w3 and the split operand `a` names (also the Judge's cat_audio_proj, on this encoder's mask)
  Status linear(const GemmParams& p, const LinW& w, int cls, const X3Operand& a, hipStream_t st) const {
    return x3_linear(p, w, cls, x3(cls), bf16_, a, who_.c_str(), "", st);
  }
  int dim() const { return d_.dim; }
  int in_dim() const { return d_.in_dim; }

 private:
  samaudio_peav_dims d_;
  bool bf16_;
  size_t esz_;
  std::string prefix_, who_;   // who_ = prefix_ + ": ", what the messages of linear start with
  bool ready_ = false;
  int x3_ = 0;
  struct LayerW {
    const float *attn_norm, *ffn_norm, *q_norm, *k_norm, *bqkv, *bo;
    LinW wqkv, wo, w13, w2;
    const float *attn_gs, *ffn_gs;   // x3: the constant [gain | shift 0] tables "<norm>.gs" [2, D] of launch_rmsnorm_gs_split3
  };
  std::vector<LayerW> layers_;
  struct {
    const void* in_w;
    LinW conv1, conv2, out;   // (x3 twins: the convolutions per tap [D, 3 taps x 3D], out.w [D, 3D])
    const float *in_b, *cls, *gn1_w, *gn1_b, *gn2_w, *gn2_b, *conv1_b, *conv2_b, *norm, *rope_cos, *rope_sin;
    const float* norm_gs;
  } g_{};
  struct {
    float *h0, *r1, *h, *out;
    void *out_act, *xn, *qkv, *Q, *K, *Vt, *attn, *u, *gnbuf;
    unsigned char* mask_s;
    double* gn_part;
    // x3 split scratch (16-bit; null / 0 unless a class that needs it is on): D-wide rows, the SwiGLU hidden, the 3x-wide halo buffer
    // of the convolutions, the attention's split output
    void *x3a, *x3u, *gn3, *attn3;
    size_t x3a_bytes, x3u_bytes, gn3_bytes, attn3_bytes;
  } w_{};
};

class Judge {
 public:
  explicit Judge(const samaudio_judge_config& c);
  Status set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape);
  Status finalize();
  Status set_option(int option, int value);   // SAMAUDIO_OPT_X3_CLASSES (fp32 contexts, before finalize)
  size_t workspace_bytes(int inputs, int candidates, int frames);
  Status set_workspace(void* p, size_t bytes);
  // reference judge.py:90-132 with the mixture branch evaluated once per clip instead of once per candidate
  // (ranking/judge.py:31-33 repeats it; every op is per-row, so this is exact):
  //   input_latent [inputs, frames, codec_dim], separated_latent [inputs*candidates, frames, codec_dim] f32,
  //   text_pooled [inputs*candidates, text_hidden] f32, pad_mask [inputs, frames] u8 or null,
  //   scores [inputs*candidates, 4] f32 = (overall, recall, precision, faithfulness)
  Status score(const float* input_latent, const float* separated_latent, int inputs, int candidates, int frames,
               const float* text_pooled, const unsigned char* pad_mask, float* scores, hipStream_t st);
  // test hook: one transformer alone; x [rows, frames, in_dim] f32 -> hidden [rows, frames + 1, dim] f32
  Status encode(int which, const float* x, const unsigned char* pad_mask, int rows, int frames, float* hidden,
                hipStream_t st);

 private:
  void plan(Bump& b, int inputs, int candidates, int frames, bool assign);
  samaudio_judge_config cfg_;
  bool bf16_;
  size_t esz_;
  int at_dtype_;
  Registry reg_;
  PeavEncoder enc_, fin_;
  int x3_ = 0;
  bool ready_ = false;
  char* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  struct {
    LinW cat_wh, cat_wi;   // (x3, class WO: "cat.wh.x3" / "cat.wi.x3" [Bn, 3D])
    const void *tp1_w, *tp2_w, *pat_wa, *pat_wt;
    const float *cat_b, *tp2_b, *ln_w, *ln_b, *pat_b, *head_w, *mean, *std_;
  } g_{};
  struct {
    void *xa, *audio, *tp_act, *t1, *tl, *at;
    float *inp_part, *t2, *tpart;
    unsigned char* mask;
  } w_{};
};

class FramePredictor {  // PE-A-Frame span predictor: per-frame audio-text logits for batch-paired rows
 public:
  explicit FramePredictor(const samaudio_frame_config& c);
  Status set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape);
  Status finalize();
  Status set_option(int option, int value);   // SAMAUDIO_OPT_X3_CLASSES (fp32 contexts, before finalize)
  size_t workspace_bytes(int rows, int frames);
  Status set_workspace(void* p, size_t bytes);
  // codec_features [rows, frames, codec_dim] f32, text_pooled [rows, embed_dim] f32, pad_mask [rows, frames] u8 or
  // null -> logits [rows, frames] f32
  Status logits(const float* codec_features, const float* text_pooled, const unsigned char* pad_mask, int rows,
                int frames, float* out, hipStream_t st);

 private:
  void plan(Bump& b, int rows, int frames, bool assign);
  samaudio_frame_config cfg_;
  bool bf16_;
  size_t esz_;
  int at_dtype_;
  Registry reg_;
  PeavEncoder enc_;
  int x3_ = 0;
  bool ready_ = false;
  char* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  struct {
    const void *ah_w, *th_w;
    const float *ah_ln_w, *ah_ln_b, *th_ln_w, *th_ln_b, *scale, *bias;
  } g_{};
  struct {
    void *xa, *a_ln, *t_ln;
    float *a_emb, *t_emb;
  } w_{};
};

}  // namespace sa
