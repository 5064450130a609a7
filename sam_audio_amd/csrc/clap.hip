// CLAP ranker towers: host code that sequences kernels of gemm.hip / peav_kernels.hip / vit_kernels.hip / t5_kernels.hip /
// kernels.hip (clap_logmel) / clap_kernels.hip, and its C entry points (include/samaudio.h "CLAP ranker towers").  "hf:" =
// transformers' modeling_clap.py, the definition every step below is checked against (tests/test_clap_gpu.py).
#include "clap.h"

#include <cmath>

struct samaudio_clap {
  sa::ClapTower* tower;
};

namespace sa {

namespace {
constexpr float kNnLayerNormEps = 1e-5f;   // the patch, merge and final norms are nn.LayerNorm(dim) with its default eps
bool k32(long k) { return k > 0 && k % 32 == 0; }   // the fp32 GEMM's K granule
}  // namespace

ClapTower::ClapTower(const samaudio_clap_config& c) : cfg_(c) {}

Status ClapTower::set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape) {
  ready_ = false;
  return reg_.set(name, p, dtype, ndim, shape);
}

Status ClapTower::finalize() {
  const samaudio_clap_config& c = cfg_;
  if (!launch_clap_patch_embed || !launch_swin_window_attn || !launch_swin_patch_merge || !launch_clap_text_embed || !launch_clap_logmel)
    return fail(SAMAUDIO_ERR_STATE, "clap: not in this build of the library");
  if (c.num_stages < 1 || c.num_stages > 4 || c.embed_dim < 1 || c.window_size < 1 || c.mlp_ratio < 1 || c.projection_dim < 1 ||
      c.spec_size < 1 || c.num_mel_bins < 1 || c.patch_stride < 1 || c.patch_size < c.patch_stride || c.hop < 1 || c.max_length < 1)
    return fail(SAMAUDIO_ERR_ARG, "clap: non-positive dimension");
  if (c.spec_size % c.num_mel_bins || c.spec_size % c.patch_stride || c.patch_size * c.patch_size > 64 || c.embed_dim > 1024)
    return fail(SAMAUDIO_ERR_ARG, "clap: spec_size must be a multiple of num_mel_bins and patch_stride; patch_size^2 <= 64, embed_dim <= 1024");
  if (frames() < 2 || frames() > c.spec_size * (c.spec_size / c.num_mel_bins))
    return fail(SAMAUDIO_ERR_ARG, "clap: 1 + max_length / hop frames exceed spec_size * freq_ratio");
  if (c.window_size * c.window_size > 64) return fail(SAMAUDIO_ERR_ARG, "clap: window_size^2 must be <= 64");
  int res = grid();
  for (int s = 0; s < c.num_stages; ++s) {
    const long C = (long)c.embed_dim << s;
    if (c.depths[s] < 1 || c.heads[s] < 1 || C % c.heads[s]) return fail(SAMAUDIO_ERR_ARG, "clap: depths / heads of a stage");
    const long hd = C / c.heads[s];
    if (hd != 24 && hd != 32) return fail(SAMAUDIO_ERR_ARG, "clap: head width must be 24 or 32");
    if (!k32(C) || !k32(C * c.mlp_ratio))
      return fail(SAMAUDIO_ERR_ARG, "clap: stage " + std::to_string(s) + ": width " + std::to_string(C) + " (a GEMM's K) must be a multiple of 32");
    if (res < c.window_size || res % c.window_size)   // (hf gathers the bias for window_size^2 tokens: a smaller map breaks there too)
      return fail(SAMAUDIO_ERR_ARG, "clap: a stage's resolution must be a multiple of window_size");
    if (s + 1 < c.num_stages) {
      if (res & 1) return fail(SAMAUDIO_ERR_ARG, "clap: odd resolution in front of a patch merge");
      res /= 2;
    }
  }
  const long Cl = (long)c.embed_dim << (c.num_stages - 1);
  if (!k32(c.projection_dim)) return fail(SAMAUDIO_ERR_ARG, "clap: projection_dim (a GEMM's K) must be a multiple of 32");
  if (c.text_vocab < 1 || c.text_hidden < 1 || c.text_heads < 1 || c.text_layers < 0 || c.text_intermediate < 1 || c.text_pad_id < 0)
    return fail(SAMAUDIO_ERR_ARG, "clap: non-positive text dimension");
  if (!k32(c.text_hidden) || !k32(c.text_intermediate) || c.text_hidden % c.text_heads)
    return fail(SAMAUDIO_ERR_ARG, "clap: text_hidden and text_intermediate (a GEMM's K) must be multiples of 32, text_hidden of text_heads");
  if (c.text_hidden / c.text_heads > 128) return fail(SAMAUDIO_ERR_ARG, "clap: text head width must be <= 128");
  if (c.text_max_positions > 514 || c.text_max_positions < c.text_pad_id + 2)
    return fail(SAMAUDIO_ERR_ARG, "clap: text_max_positions must be in [text_pad_id + 2, 514]");

  const int N = c.fft_size, F = c.num_mel_bins, E = c.projection_dim, PP = c.patch_size * c.patch_size;
  NEEDF(reg_, g_.tables, "fe.tables", 2 * N);
  NEEDF(reg_, g_.bank, "fe.bank", N / 2 + 1, F);
  NEEDF(reg_, g_.bn_scale, "fe.bn_scale", F);
  NEEDF(reg_, g_.bn_shift, "fe.bn_shift", F);
  NEEDF(reg_, g_.patch_w, "a.patch.w", c.embed_dim, PP);
  NEEDF(reg_, g_.patch_b, "a.patch.b", c.embed_dim);
  g_.patch_ln_w = g_.patch_ln_b = nullptr;
  if (c.patch_norm) {
    NEEDF(reg_, g_.patch_ln_w, "a.patch.ln_w", c.embed_dim);
    NEEDF(reg_, g_.patch_ln_b, "a.patch.ln_b", c.embed_dim);
  }
  stages_.assign(c.num_stages, StageW{});
  for (int s = 0; s < c.num_stages; ++s) {
    const long C = (long)c.embed_dim << s, Fm = C * c.mlp_ratio, span = 2 * c.window_size - 1;
    StageW& sw = stages_[s];
    sw.blocks.assign(c.depths[s], BlockW{});
    for (int i = 0; i < c.depths[s]; ++i) {
      const std::string L = "a.S" + std::to_string(s) + ".B" + std::to_string(i) + ".";
      BlockW& w = sw.blocks[i];
      NEEDF(reg_, w.ln1_w, L + "ln1_w", C);
      NEEDF(reg_, w.ln1_b, L + "ln1_b", C);
      NEEDF(reg_, w.qkv.w, L + "wqkv", 3 * C, C);
      NEEDF(reg_, w.qkv.b, L + "bqkv", 3 * C);
      NEEDF(reg_, w.rpb, L + "rpb", span * span, c.heads[s]);
      NEEDF(reg_, w.o.w, L + "wo", C, C);
      NEEDF(reg_, w.o.b, L + "bo", C);
      NEEDF(reg_, w.ln2_w, L + "ln2_w", C);
      NEEDF(reg_, w.ln2_b, L + "ln2_b", C);
      NEEDF(reg_, w.fc1.w, L + "w1", Fm, C);
      NEEDF(reg_, w.fc1.b, L + "b1", Fm);
      NEEDF(reg_, w.fc2.w, L + "w2", C, Fm);
      NEEDF(reg_, w.fc2.b, L + "b2", C);
    }
    if (s + 1 < c.num_stages) {
      const std::string L = "a.S" + std::to_string(s) + ".merge.";
      NEEDF(reg_, sw.merge_ln_w, L + "ln_w", 4 * C);
      NEEDF(reg_, sw.merge_ln_b, L + "ln_b", 4 * C);
      NEEDF(reg_, sw.merge_w, L + "w", 2 * C, 4 * C);
    }
  }
  NEEDF(reg_, g_.norm_w, "a.norm_w", Cl);
  NEEDF(reg_, g_.norm_b, "a.norm_b", Cl);
  NEEDF(reg_, g_.aproj1.w, "a.proj.w1", E, Cl);
  NEEDF(reg_, g_.aproj1.b, "a.proj.b1", E);
  NEEDF(reg_, g_.aproj2.w, "a.proj.w2", E, E);
  NEEDF(reg_, g_.aproj2.b, "a.proj.b2", E);

  const long D = c.text_hidden, Ft = c.text_intermediate;
  NEEDF(reg_, g_.word, "t.word", c.text_vocab, D);
  NEEDF(reg_, g_.pos, "t.pos", c.text_max_positions, D);
  NEEDF(reg_, g_.type, "t.type", D);
  NEEDF(reg_, g_.emb_ln_w, "t.emb_ln_w", D);
  NEEDF(reg_, g_.emb_ln_b, "t.emb_ln_b", D);
  text_.assign(c.text_layers, TextLayerW{});
  for (int i = 0; i < c.text_layers; ++i) {
    const std::string L = "t.L" + std::to_string(i) + ".";
    TextLayerW& w = text_[i];
    NEEDF(reg_, w.qkv.w, L + "wqkv", 3 * D, D);
    NEEDF(reg_, w.qkv.b, L + "bqkv", 3 * D);
    NEEDF(reg_, w.o.w, L + "wo", D, D);
    NEEDF(reg_, w.o.b, L + "bo", D);
    NEEDF(reg_, w.ln1_w, L + "ln1_w", D);
    NEEDF(reg_, w.ln1_b, L + "ln1_b", D);
    NEEDF(reg_, w.fc1.w, L + "w1", Ft, D);
    NEEDF(reg_, w.fc1.b, L + "b1", Ft);
    NEEDF(reg_, w.fc2.w, L + "w2", D, Ft);
    NEEDF(reg_, w.fc2.b, L + "b2", D);
    NEEDF(reg_, w.ln2_w, L + "ln2_w", D);
    NEEDF(reg_, w.ln2_b, L + "ln2_b", D);
  }
  NEEDF(reg_, g_.pool.w, "t.pool.w", D, D);
  NEEDF(reg_, g_.pool.b, "t.pool.b", D);
  NEEDF(reg_, g_.tproj1.w, "t.proj.w1", E, D);
  NEEDF(reg_, g_.tproj1.b, "t.proj.b1", E);
  NEEDF(reg_, g_.tproj2.w, "t.proj.w2", E, E);
  NEEDF(reg_, g_.tproj2.b, "t.proj.b2", E);
  ready_ = true;
  return Status{};
}

// stage 0 is the widest point of every buffer: a merge quarters the tokens and doubles the width
void ClapTower::plan_audio(Bump& b, long n, AudioWs* w) const {
  const long T0 = (long)grid() * grid(), C0 = cfg_.embed_dim, Cl = C0 << (cfg_.num_stages - 1), M = n * T0;
  AudioWs a;
  a.feat = (float*)b.take((size_t)n * frames() * cfg_.num_mel_bins * 4);
  a.h = (float*)b.take((size_t)M * C0 * 4);
  a.xn = (float*)b.take((size_t)M * C0 * 4);
  a.qkv = (float*)b.take((size_t)M * 3 * C0 * 4);
  a.attn = (float*)b.take((size_t)M * C0 * 4);
  a.u = (float*)b.take((size_t)M * cfg_.mlp_ratio * C0 * 4);
  a.pooled = (float*)b.take((size_t)n * Cl * 4);
  a.p1 = (float*)b.take((size_t)n * cfg_.projection_dim * 4);
  if (w) *w = a;
}

void ClapTower::plan_text(Bump& b, long rows, long tokens, TextWs* w) const {
  const long M = rows * tokens, D = cfg_.text_hidden;
  TextWs t;
  t.e = (float*)b.take((size_t)M * D * 4);
  t.h = (float*)b.take((size_t)M * D * 4);
  t.y = (float*)b.take((size_t)M * D * 4);
  t.qkv = (float*)b.take((size_t)M * 3 * D * 4);
  t.attn = (float*)b.take((size_t)M * D * 4);
  t.u = (float*)b.take((size_t)M * cfg_.text_intermediate * 4);
  t.pooled = (float*)b.take((size_t)rows * D * 4);
  t.p1 = (float*)b.take((size_t)rows * cfg_.projection_dim * 4);
  if (w) *w = t;
}

size_t ClapTower::workspace_bytes(int audio_rows, int text_rows, int tokens) {
  size_t need = 0;
  if (audio_rows > 0) {
    Bump b;
    plan_audio(b, audio_rows, nullptr);
    need = b.used();
  }
  if (text_rows > 0 && tokens > 0) {
    Bump b;
    plan_text(b, text_rows, tokens, nullptr);
    need = b.used() > need ? b.used() : need;
  }
  return need;
}

Status ClapTower::set_workspace(void* p, size_t bytes) {
  if (!p || (reinterpret_cast<uintptr_t>(p) & 255)) return fail(SAMAUDIO_ERR_WORKSPACE, "clap: workspace must be 256-byte aligned");
  ws_ = (char*)p;
  ws_bytes_ = bytes;
  return Status{};
}

namespace {
// y = act(x W^T + b) [+ res]: out may be res (the residual stream is updated in place)
Status linear(const float* x, long K, const float* w, const float* b, long M, long N, int act, const float* res, float* out,
              hipStream_t st, long lda = 0) {
  GemmParams p = lin(x, lda ? lda : K, w, M, (int)N, (int)K);
  p.bias = b;
  if (act != ACT_NONE) {
    p.act = act;
    p.out_act = out; p.act_ld = N;
  } else {
    p.res = res; p.res_ld = N;
    p.out_f32 = out; p.f32_ld = N;
  }
  return run_gemm(p, false, "clap: ", st);
}
}  // namespace

Status ClapTower::audio_embed(const float* wav, int rows, long row_stride, const int64_t* lengths, const int64_t* offsets, bool quantise,
                              float* out, hipStream_t st) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, "clap: weights not finalized");
  if (!wav || !lengths || !out || rows <= 0) return fail(SAMAUDIO_ERR_ARG, "clap: audio_embed: null argument or rows < 1");
  if (!ws_) return fail(SAMAUDIO_ERR_WORKSPACE, "clap: no workspace");
  const samaudio_clap_config& c = cfg_;
  AudioWs w;
  Bump bump(ws_, ws_bytes_);
  plan_audio(bump, rows, &w);
  if (!bump.fits()) return fail(SAMAUDIO_ERR_WORKSPACE, "clap: workspace too small for " + std::to_string(rows) + " clips");
  // hf: ClapFeatureExtractor, then ClapAudioEncoder.batch_norm (eval mode: a scale and a shift per mel bin)
  const int rc = samaudio_op_logmel(wav, rows, row_stride, lengths, offsets, c.max_length, quantise ? 1 : 0, c.fft_size, c.hop,
                                    c.num_mel_bins, g_.tables, g_.bank, g_.bn_scale, g_.bn_shift, w.feat, (samaudio_stream)st);
  if (rc != SAMAUDIO_OK) return fail(rc, std::string("clap: ") + samaudio_last_error());
  // hf: reshape_mel2img + ClapAudioPatchEmbed
  SA_HIP(launch_clap_patch_embed(w.feat, rows, frames(), c.num_mel_bins, c.spec_size, c.patch_size, c.patch_stride, c.embed_dim,
                                 g_.patch_w, g_.patch_b, g_.patch_ln_w, g_.patch_ln_b, kNnLayerNormEps, w.h, st));
  int res = grid();
  long C = c.embed_dim;
  for (int s = 0; s < c.num_stages; ++s) {   // hf: ClapAudioStage
    const long M = (long)rows * res * res, Fm = C * c.mlp_ratio;
    const int heads = c.heads[s], hd = (int)(C / heads);
    for (int i = 0; i < c.depths[s]; ++i) {  // hf: ClapAudioLayer
      const BlockW& bw = stages_[s].blocks[i];
      // hf: set_shift_and_window_size - a map no larger than the window is one unshifted window
      const int shift = (i % 2 == 1 && res > c.window_size) ? c.window_size / 2 : 0;
      SA_HIP(launch_layernorm_rows(w.h, C, bw.ln1_w, bw.ln1_b, w.xn, nullptr, false, M, (int)C, c.audio_ln_eps, st));
      SA_TRY(linear(w.xn, C, bw.qkv.w, bw.qkv.b, M, 3 * C, ACT_NONE, nullptr, w.qkv, st));
      SA_HIP(launch_swin_window_attn(w.qkv, bw.rpb, w.attn, rows, res, res, heads, hd, c.window_size, shift, st));
      SA_TRY(linear(w.attn, C, bw.o.w, bw.o.b, M, C, ACT_NONE, w.h, w.h, st));
      SA_HIP(launch_layernorm_rows(w.h, C, bw.ln2_w, bw.ln2_b, w.xn, nullptr, false, M, (int)C, c.audio_ln_eps, st));
      SA_TRY(linear(w.xn, C, bw.fc1.w, bw.fc1.b, M, Fm, ACT_GELU, nullptr, w.u, st));
      SA_TRY(linear(w.u, Fm, bw.fc2.w, bw.fc2.b, M, C, ACT_NONE, w.h, w.h, st));
    }
    if (s + 1 < c.num_stages) {  // hf: ClapAudioPatchMerging
      SA_HIP(launch_swin_patch_merge(w.h, stages_[s].merge_ln_w, stages_[s].merge_ln_b, kNnLayerNormEps, w.xn, rows, res, res, (int)C, st));
      SA_TRY(linear(w.xn, 4 * C, stages_[s].merge_w, nullptr, M / 4, 2 * C, ACT_NONE, nullptr, w.h, st));
      res /= 2;
      C *= 2;
    }
  }
  // hf: self.norm, then modeling_clap.py:878-895 - permute(0, 2, 1) and reshape to [C, freq, time], split freq into (ratio, c_freq_bin),
  // permute, flatten(2), AdaptiveAvgPool1d(1): every step moves tokens around within a channel and the pool averages ALL of a channel's
  // tokens, so the result is the mean over the tokens, whatever their order
  const long T = (long)res * res;
  SA_HIP(launch_layernorm_rows(w.h, C, g_.norm_w, g_.norm_b, w.xn, nullptr, false, rows * T, (int)C, kNnLayerNormEps, st));
  SA_HIP(launch_token_mean(w.xn, C, w.pooled, nullptr, false, rows, (int)T, (int)C, st));
  // hf: ClapProjectionLayer, F.normalize
  SA_TRY(linear(w.pooled, C, g_.aproj1.w, g_.aproj1.b, rows, c.projection_dim, ACT_RELU, nullptr, w.p1, st));
  SA_TRY(linear(w.p1, c.projection_dim, g_.aproj2.w, g_.aproj2.b, rows, c.projection_dim, ACT_NONE, nullptr, out, st));
  SA_HIP(launch_l2_normalize(out, rows, c.projection_dim, st));
  return Status{};
}

Status ClapTower::text_embed(const long long* ids, const unsigned char* mask, int rows, int tokens, float* out, hipStream_t st) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, "clap: weights not finalized");
  if (!ids || !mask || !out || rows <= 0 || tokens <= 0) return fail(SAMAUDIO_ERR_ARG, "clap: text_embed: bad argument");
  const samaudio_clap_config& c = cfg_;
  if (tokens > 512) return fail(SAMAUDIO_ERR_ARG, "clap: more than 512 tokens (launch_t5_attention)");
  if (tokens + c.text_pad_id + 1 > c.text_max_positions)
    return fail(SAMAUDIO_ERR_ARG, "clap: " + std::to_string(tokens) + " tokens exceed the position table (text_max_positions " +
                                      std::to_string(c.text_max_positions) + ", positions start at text_pad_id + 1)");
  if (!ws_) return fail(SAMAUDIO_ERR_WORKSPACE, "clap: no workspace");
  TextWs w;
  Bump bump(ws_, ws_bytes_);
  plan_text(bump, rows, tokens, &w);
  if (!bump.fits()) return fail(SAMAUDIO_ERR_WORKSPACE, "clap: workspace too small for " + std::to_string((long)rows * tokens) + " token rows");
  const long M = (long)rows * tokens, D = c.text_hidden, Ft = c.text_intermediate;
  const int H = c.text_heads, hd = (int)(D / H);
  const float eps = c.text_ln_eps;
  // hf: ClapTextEmbeddings
  SA_HIP(launch_clap_text_embed(ids, g_.word, g_.pos, g_.type, w.e, rows, tokens, (int)D, c.text_vocab, c.text_pad_id, st));
  SA_HIP(launch_layernorm_rows(w.e, D, g_.emb_ln_w, g_.emb_ln_b, w.h, nullptr, false, M, (int)D, eps, st));
  for (const TextLayerW& lw : text_) {   // hf: ClapTextLayer (post-LN)
    SA_TRY(linear(w.h, D, lw.qkv.w, lw.qkv.b, M, 3 * D, ACT_NONE, nullptr, w.qkv, st));
    SA_HIP(launch_t5_attention(w.qkv, mask, nullptr, w.attn, false, rows, tokens, H, hd, 512, 1.0f / std::sqrt((float)hd), 0, st));
    SA_TRY(linear(w.attn, D, lw.o.w, lw.o.b, M, D, ACT_NONE, w.h, w.y, st));
    SA_HIP(launch_layernorm_rows(w.y, D, lw.ln1_w, lw.ln1_b, w.h, nullptr, false, M, (int)D, eps, st));
    SA_TRY(linear(w.h, D, lw.fc1.w, lw.fc1.b, M, Ft, ACT_GELU, nullptr, w.u, st));
    SA_TRY(linear(w.u, Ft, lw.fc2.w, lw.fc2.b, M, D, ACT_NONE, w.h, w.y, st));
    SA_HIP(launch_layernorm_rows(w.y, D, lw.ln2_w, lw.ln2_b, w.h, nullptr, false, M, (int)D, eps, st));
  }
  // hf: ClapTextPooler - dense + tanh on token 0 of every row (A rows tokens * D apart); ClapProjectionLayer; F.normalize
  SA_TRY(linear(w.h, D, g_.pool.w, g_.pool.b, rows, D, ACT_TANH, nullptr, w.pooled, st, (long)tokens * D));
  SA_TRY(linear(w.pooled, D, g_.tproj1.w, g_.tproj1.b, rows, c.projection_dim, ACT_RELU, nullptr, w.p1, st));
  SA_TRY(linear(w.p1, c.projection_dim, g_.tproj2.w, g_.tproj2.b, rows, c.projection_dim, ACT_NONE, nullptr, out, st));
  SA_HIP(launch_l2_normalize(out, rows, c.projection_dim, st));
  return Status{};
}

}  // namespace sa

extern "C" {

int samaudio_clap_create(const samaudio_clap_config* cfg, samaudio_clap** out) {
  if (!cfg || !out) return sa::bad("samaudio_clap_create: null argument");
  if (cfg->enable_fusion) return sa::bad("samaudio_clap_create: enable_fusion=True (feature fusion) is not built: the ranker uses the unfused model");
  samaudio_clap* t = new samaudio_clap;
  t->tower = new sa::ClapTower(*cfg);
  *out = t;
  return SAMAUDIO_OK;
}

void samaudio_clap_destroy(samaudio_clap* t) {
  if (!t) return;
  delete t->tower;
  delete t;
}

int samaudio_clap_set_tensor(samaudio_clap* t, const char* name, const void* data, int dtype, int ndim, const int64_t* shape) {
  return SA_ENTRY(t, "null clap tower", t->tower->set_tensor(name, data, dtype, ndim, shape));
}

int samaudio_clap_finalize(samaudio_clap* t) { return SA_ENTRY(t, "null clap tower", t->tower->finalize()); }

size_t samaudio_clap_workspace_bytes(samaudio_clap* t, int audio_rows, int text_rows, int tokens) {
  if (!t) return 0;
  return t->tower->workspace_bytes(audio_rows, text_rows, tokens);
}

int samaudio_clap_set_workspace(samaudio_clap* t, void* workspace, size_t bytes) {
  return SA_ENTRY(t, "null clap tower", t->tower->set_workspace(workspace, bytes));
}

int samaudio_clap_audio_embed(samaudio_clap* t, const float* wav, int rows, int64_t row_stride, const int64_t* lengths,
                              const int64_t* offsets, int quantise, float* out, samaudio_stream stream) {
  return SA_ENTRY(t, "null clap tower",
                  t->tower->audio_embed(wav, rows, (long)row_stride, lengths, offsets, quantise != 0, out, (hipStream_t)stream));
}

int samaudio_clap_text_embed(samaudio_clap* t, const int64_t* input_ids, const unsigned char* attention_mask, int rows, int tokens,
                             float* out, samaudio_stream stream) {
  return SA_ENTRY(t, "null clap tower",
                  t->tower->text_embed((const long long*)input_ids, attention_mask, rows, tokens, out, (hipStream_t)stream));
}

int samaudio_clap_score(const float* audio, const float* text, int clips, int candidates, int dim, float* scores,
                        samaudio_stream stream) {
  if (!audio || !text || !scores || clips < 1 || candidates < 1 || dim < 1) return sa::bad("clap_score: null argument / clips, candidates, dim < 1");
  if (!sa::launch_clap_score) {
    sa::set_last_error("clap_score: not in this build of the library");
    return SAMAUDIO_ERR_STATE;
  }
  const hipError_t e = sa::launch_clap_score(audio, text, scores, clips, candidates, dim, (hipStream_t)stream);
  if (e == hipSuccess) return SAMAUDIO_OK;
  sa::set_last_error(std::string("clap_score: ") + hipGetErrorString(e));
  return SAMAUDIO_ERR_HIP;
}

int samaudio_op_clap_patch_embed(const float* feat, int n, int frames, int n_mels, int spec_size, int patch_size, int patch_stride,
                                 int dim, const float* w, const float* bias, const float* ln_w, const float* ln_b, float eps,
                                 float* tokens, samaudio_stream stream) {
  if (!feat || !w || !bias || !tokens || (ln_w == nullptr) != (ln_b == nullptr)) return sa::bad("clap_patch_embed: null argument");
  if (n < 1 || n_mels < 1 || spec_size < 1 || patch_stride < 1 || patch_size < patch_stride || patch_size * patch_size > 64 || dim < 1 ||
      dim > 1024 || spec_size % n_mels || spec_size % patch_stride || frames < 2 || frames > spec_size * (spec_size / n_mels))
    return sa::bad("clap_patch_embed: dims (spec_size % n_mels, spec_size % patch_stride, patch_size^2 <= 64, dim <= 1024, 2 <= frames <= spec_size * freq_ratio)");
  if (!sa::launch_clap_patch_embed) {
    sa::set_last_error("clap_patch_embed: not in this build of the library");
    return SAMAUDIO_ERR_STATE;
  }
  const hipError_t e = sa::launch_clap_patch_embed(feat, n, frames, n_mels, spec_size, patch_size, patch_stride, dim, w, bias, ln_w, ln_b,
                                                   eps, tokens, (hipStream_t)stream);
  if (e == hipSuccess) return SAMAUDIO_OK;
  sa::set_last_error(std::string("clap_patch_embed: ") + hipGetErrorString(e));
  return SAMAUDIO_ERR_HIP;
}

int samaudio_op_swin_window_attn(const float* qkv, const float* table, float* out, int n, int height, int width, int heads,
                                 int head_dim, int window, int shift, samaudio_stream stream) {
  if (!qkv || !table || !out) return sa::bad("swin_window_attn: null argument");
  if (n < 1 || n > 65535 || heads < 1 || window < 1 || window * window > 64 || height % window || width % window || shift < 0 ||
      shift >= window || (head_dim != 24 && head_dim != 32))
    return sa::bad("swin_window_attn: dims (head_dim 24 | 32, window^2 <= 64, height and width multiples of window, 0 <= shift < window)");
  if (!sa::launch_swin_window_attn) {
    sa::set_last_error("swin_window_attn: not in this build of the library");
    return SAMAUDIO_ERR_STATE;
  }
  const hipError_t e = sa::launch_swin_window_attn(qkv, table, out, n, height, width, heads, head_dim, window, shift, (hipStream_t)stream);
  if (e == hipSuccess) return SAMAUDIO_OK;
  sa::set_last_error(std::string("swin_window_attn: ") + hipGetErrorString(e));
  return SAMAUDIO_ERR_HIP;
}

int samaudio_op_swin_patch_merge(const float* x, const float* ln_w, const float* ln_b, float eps, float* out, int n, int height,
                                 int width, int dim, samaudio_stream stream) {
  if (!x || !ln_w || !ln_b || !out) return sa::bad("swin_patch_merge: null argument");
  if (n < 1 || height < 2 || width < 2 || (height & 1) || (width & 1) || dim < 1) return sa::bad("swin_patch_merge: n, dim < 1 or an odd map");
  if (!sa::launch_swin_patch_merge) {
    sa::set_last_error("swin_patch_merge: not in this build of the library");
    return SAMAUDIO_ERR_STATE;
  }
  const hipError_t e = sa::launch_swin_patch_merge(x, ln_w, ln_b, eps, out, n, height, width, dim, (hipStream_t)stream);
  if (e == hipSuccess) return SAMAUDIO_OK;
  sa::set_last_error(std::string("swin_patch_merge: ") + hipGetErrorString(e));
  return SAMAUDIO_ERR_HIP;
}

}  // extern "C"
