// Host-side orchestration of the PE-Core vision tower: patch embedding ->
// [class token ;] + positions -> ln_pre -> layers x { LayerNorm, fused q|k|v (+bias), 2-D RoPE, flash attention,
// out_proj (+bias, residual) ; LayerNorm, c_fc (+bias, GELU), c_proj (+bias, residual) } -> ln_post -> pooling
// (class token | mean | attention pooling head) -> projection -> optional L2 normalisation.
// Reference: sam_audio/model/vision_encoder.py:80-89 (`pe.CLIP.encode_image`); architecture restated in
// oracle/vit_oracle.py.  Like Engine it owns no device memory: borrowed weights, one caller-provided workspace.
// SAMAUDIO_OPT_X3_CLASSES of an fp32 context (mask of SAMAUDIO_CLS_X3_VIT bits, before finalize): the four GEMMs of every layer (and
// pool.wkv, with QKV) and the self-attention multiply compensated 16-bit operands; the patch embedding, ln_pre, the pooling attention,
// every n-row launch (pool.wo / w1 / w2, proj) and the L2 normalisation stay exact fp32.  0 = today's exact-fp32 launches, bit for bit.
#pragma once
#include "host.h"

namespace sa {

class VisionTower {
 public:
  explicit VisionTower(const samaudio_vit_config& c);
  Status set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape);
  Status finalize();
  Status set_option(int option, int value);   // SAMAUDIO_OPT_X3_CLASSES (fp32 contexts, before finalize; query the workspace after it)
  size_t workspace_bytes(int frames);
  Status set_workspace(void* p, size_t bytes);
  Status encode(const float* frames, int n, bool normalize, float* features, float* tokens_out, hipStream_t st);
  // the same on raw uint8 frames [n, 3, height, width]: resized (mode = SAMAUDIO_RESIZE_*), rounded and normalised by the launch that
  // writes the patch embedding's operand
  Status encode_frames(const uint8_t* frames, int n, int height, int width, int mode, bool normalize, float* features,
                       float* tokens_out, hipStream_t st);
  // ... on n frames picked from a video [src_frames, 3, height, width] by the device table `pick` (null = all of them, in order), source
  // pixels under a non-zero byte of `mask` [src_frames, mask_channels, height, width] (null = none) zeroed - both inside that launch
  Status encode_video(const uint8_t* frames, int64_t src_frames, int height, int width, const uint8_t* mask, int mask_channels,
                      const int32_t* pick, int n, int mode, bool normalize, float* features, float* tokens_out, hipStream_t st);

 private:
  void plan(Bump& b, int n, bool assign);
  Status prepare(const void* frames, const float* features, int n);   // argument / state / workspace checks, the plan for n frames
  Status encode_patches(int n, bool normalize, float* features, float* tokens_out, hipStream_t st);   // everything behind w_.patches
  bool x3(int cls) const { return (x3_ & cls) != 0; }
  // One launch on the weight `w`: `p` = the context's plain launch, run as it is on w.w - or, class `cls` switched to compensated
  // operands, as ONE 16-bit launch over K' = 3K on w.w3 and the split operand `a` names (host.h x3_linear)
  Status linear(const GemmParams& p, const LinW& w, int cls, const X3Operand& a, hipStream_t st) const {
    return x3_linear(p, w, cls, x3(cls), bf16_, a, kWho, kWho, st);
  }
  static constexpr const char* kWho = "vision tower: ";   // the prefix of the context's messages
  int tokens() const { return grid_ * grid_ + (cfg_.use_cls_token ? 1 : 0); }
  samaudio_vit_config cfg_;
  bool bf16_;
  size_t esz_;
  int at_dtype_;
  int grid_, kp_, hd_, pool_hd_;
  Registry reg_;
  bool ready_ = false;
  int x3_ = 0;
  char* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  int planned_n_ = 0;
  struct LayerW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *bqkv, *bo, *b1, *b2;
    LinW wqkv, wo, w1, w2;   // (x3 twins "L<i>.<name>.x3": [3W, 3W], [W, 3W], [F, 3W], [W, 3F])
  };
  std::vector<LayerW> layers_;
  struct {
    const void *patch_w, *proj, *pool_wo, *pool_w1, *pool_w2;
    LinW pool_wkv;   // (class QKV: "pool.wkv.x3" [2W, 3W])
    const float *pos, *ln_pre_w, *ln_pre_b, *ln_post_w, *ln_post_b, *rope_cos, *rope_sin;
    const float *pool_q, *pool_bkv, *pool_bo, *pool_ln_w, *pool_ln_b, *pool_b1, *pool_b2;
  } g_{};
  struct {
    void *patches, *xn, *qkv, *Q, *K, *Vt, *attn, *u, *kv, *pooled, *yn, *u2, *z_act;
    float *h, *y, *z;
    unsigned char* mask;
    // x3 split scratch (16-bit; null / 0 unless a class that reads it is on): W-wide rows [M, 3W] - LayerNorm output, then the
    // attention's split output / the split of its fp32 output, one after the other - and the MLP hidden [M, 3F]
    void *x3a, *x3u;
    size_t x3a_bytes, x3u_bytes;
  } w_{};
};

}  // namespace sa
