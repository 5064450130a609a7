// Host-side orchestration of the CLAP ranker towers (samaudio.h "CLAP ranker towers"; the definition is
// transformers' ClapModel without feature fusion):
//   audio  waveforms -> clap_logmel (BatchNorm folded in) -> clap_patch_embed -> stages x { blocks x { LayerNorm, fused q|k|v,
//          swin_window_attn (shifted in every second block), proj (+residual) ; LayerNorm, fc1 GELU, fc2 (+residual) },
//          swin_patch_merge + the bias-free 4 C -> 2 C reduction (all but the last stage) } -> LayerNorm -> mean over all tokens ->
//          Linear, ReLU, Linear -> L2 normalisation
//   text   ids -> clap_text_embed -> LayerNorm -> layers x { fused q|k|v, attention under the key mask, o (+residual), LayerNorm ;
//          fc1 GELU, fc2 (+residual), LayerNorm } (post-LN) -> token 0 -> dense, tanh -> Linear, ReLU, Linear -> L2 normalisation
// fp32 only: C = 96 of stage 0 is no multiple of the 16-bit kernels' K granule of 64, and the towers are under 1 % of a candidates
// step by flop count.  Like the other towers it owns no device memory: borrowed weights, one caller-provided workspace.
#pragma once
#include "host.h"

namespace sa {

class ClapTower {
 public:
  explicit ClapTower(const samaudio_clap_config& c);
  Status set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape);
  Status finalize();
  size_t workspace_bytes(int audio_rows, int text_rows, int tokens);
  Status set_workspace(void* p, size_t bytes);
  Status audio_embed(const float* wav, int rows, long row_stride, const int64_t* lengths, const int64_t* offsets, bool quantise,
                     float* out, hipStream_t st);
  Status text_embed(const long long* ids, const unsigned char* mask, int rows, int tokens, float* out, hipStream_t st);

 private:
  struct AudioWs { float *feat, *h, *xn, *qkv, *attn, *u, *pooled, *p1; };
  struct TextWs { float *e, *h, *y, *qkv, *attn, *u, *pooled, *p1; };
  void plan_audio(Bump& b, long n, AudioWs* w) const;
  void plan_text(Bump& b, long rows, long tokens, TextWs* w) const;
  int frames() const { return 1 + cfg_.max_length / cfg_.hop; }
  int grid() const { return cfg_.spec_size / cfg_.patch_stride; }
  samaudio_clap_config cfg_;
  Registry reg_;
  bool ready_ = false;
  char* ws_ = nullptr;
  size_t ws_bytes_ = 0;
  struct Lin { const float *w, *b; };
  struct BlockW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *rpb;
    Lin qkv, o, fc1, fc2;
  };
  struct StageW {
    std::vector<BlockW> blocks;
    const float *merge_ln_w = nullptr, *merge_ln_b = nullptr, *merge_w = nullptr;
  };
  std::vector<StageW> stages_;
  struct TextLayerW {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    Lin qkv, o, fc1, fc2;
  };
  std::vector<TextLayerW> text_;
  struct {
    const float *tables, *bank, *bn_scale, *bn_shift;
    const float *patch_w, *patch_b, *patch_ln_w, *patch_ln_b, *norm_w, *norm_b;
    Lin aproj1, aproj2;
    const float *word, *pos, *type, *emb_ln_w, *emb_ln_b;
    Lin pool, tproj1, tproj2;
  } g_{};
};

}  // namespace sa
