// PE-Core vision tower: host code that sequences kernels of gemm*.hip / attention.hip / peav_kernels.hip /
// vit_kernels.hip, and its C entry points (include/samaudio.h "visual-prompt tower").  "oracle:" = oracle/vit_oracle.py,
// the CPU restatement of the published architecture every step below is checked against.
#include "vit.h"

#include <cstring>

struct samaudio_vit {
  sa::VisionTower* tower;
};

namespace sa {

VisionTower::VisionTower(const samaudio_vit_config& c)
    : cfg_(c), bf16_(c.precision == SAMAUDIO_BF16), esz_(bf16_ ? 2 : 4),
      at_dtype_(bf16_ ? SAMAUDIO_DT_BF16 : SAMAUDIO_DT_F32) {
  grid_ = c.patch_size > 0 ? c.image_size / c.patch_size : 0;
  kp_ = (int)round_up(3L * c.patch_size * c.patch_size, 64);
  hd_ = c.heads > 0 ? c.width / c.heads : 0;
  pool_hd_ = c.pool_heads > 0 ? c.width / c.pool_heads : 0;
}

Status VisionTower::set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape) {
  ready_ = false;
  return reg_.set(name, p, dtype, ndim, shape);
}

Status VisionTower::set_option(int option, int value) {
  if (option != SAMAUDIO_OPT_X3_CLASSES) return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_set_option: unknown option");
  if (bf16_)
    return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_set_option: SAMAUDIO_OPT_X3_CLASSES applies to fp32 contexts (compensated 16-bit operands under fp32 storage)");
  if (value & ~SAMAUDIO_CLS_X3_VIT)
    return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_set_option: SAMAUDIO_OPT_X3_CLASSES: only qkv, wo, w13, w2 and SAMAUDIO_X3_ATTENTION");
  x3_ = value;
  ready_ = false;     // finalize resolves the twins of the switched classes
  planned_n_ = 0;     // ... and the workspace plan holds the split scratch of the classes that are on
  return Status{};
}

Status VisionTower::finalize() {
  const samaudio_vit_config& c = cfg_;
  if (c.image_size <= 0 || c.patch_size <= 0 || c.image_size % c.patch_size || c.width <= 0 || c.layers < 0 ||
      c.heads <= 0 || c.mlp_width <= 0 || c.output_dim <= 0)
    return fail(SAMAUDIO_ERR_ARG, "vision tower: non-positive dimension / image_size % patch_size");
  if (c.width % 64 || c.mlp_width % 64 || c.output_dim % 4)
    return fail(SAMAUDIO_ERR_ARG, "vision tower: width / mlp_width must be multiples of 64, output_dim of 4");
  if (c.width % c.heads || (hd_ != 64 && hd_ != 128)) return fail(SAMAUDIO_ERR_ARG, "vision tower: head dim must be 64 or 128");
  if (c.pool_type < 0 || c.pool_type > 2) return fail(SAMAUDIO_ERR_ARG, "vision tower: pool_type");
  if (c.pool_type == 0 && !c.use_cls_token) return fail(SAMAUDIO_ERR_ARG, "vision tower: class-token pooling without a class token");
  if (c.pool_type == 2 && (c.pool_heads <= 0 || c.width % c.pool_heads || (pool_hd_ != 64 && pool_hd_ != 128)))
    return fail(SAMAUDIO_ERR_ARG, "vision tower: pooling head dim must be 64 or 128");
  if (c.act != ACT_GELU && c.act != ACT_QUICK_GELU) return fail(SAMAUDIO_ERR_ARG, "vision tower: act must be 4 (gelu) or 5 (quick gelu)");
  const int W = c.width, F = c.mlp_width, S = tokens();
  const int AT = at_dtype_;
  NEEDW(reg_, AT, g_.patch_w, "patch.w", W, kp_);        // conv1.weight [W,3,P,P] flattened, K zero-padded to a multiple of 64
  NEEDF(reg_, g_.pos, "pos", S, W);                  // positional_embedding (zeros without it); row 0 += class_embedding
  g_.ln_pre_w = g_.ln_pre_b = g_.ln_post_w = g_.ln_post_b = g_.rope_cos = g_.rope_sin = nullptr;
  if (c.use_ln_pre) { NEEDF(reg_, g_.ln_pre_w, "ln_pre.w", W); NEEDF(reg_, g_.ln_pre_b, "ln_pre.b", W); }
  if (c.use_ln_post) { NEEDF(reg_, g_.ln_post_w, "ln_post.w", W); NEEDF(reg_, g_.ln_post_b, "ln_post.b", W); }
  if (c.use_rope2d) { NEEDF(reg_, g_.rope_cos, "rope_cos", S, hd_ / 2); NEEDF(reg_, g_.rope_sin, "rope_sin", S, hd_ / 2); }
  layers_.assign(c.layers, LayerW{});
  for (int i = 0; i < c.layers; ++i) {
    const std::string L = "L" + std::to_string(i) + ".";
    LayerW& w = layers_[i];
    NEEDF(reg_, w.ln1_w, L + "ln1.w", W); NEEDF(reg_, w.ln1_b, L + "ln1.b", W);
    NEEDW(reg_, AT, w.wqkv.w, L + "wqkv", 3 * W, W); NEEDF(reg_, w.bqkv, L + "bqkv", 3 * W);
    NEEDW(reg_, AT, w.wo.w, L + "wo", W, W); NEEDF(reg_, w.bo, L + "bo", W);
    NEEDF(reg_, w.ln2_w, L + "ln2.w", W); NEEDF(reg_, w.ln2_b, L + "ln2.b", W);
    NEEDW(reg_, AT, w.w1.w, L + "w1", F, W); NEEDF(reg_, w.b1, L + "b1", F);
    NEEDW(reg_, AT, w.w2.w, L + "w2", W, F); NEEDF(reg_, w.b2, L + "b2", W);
    // SAMAUDIO_OPT_X3_CLASSES: the twins [W_hi | W_lo | W_hi] of the classes that are switched on
    if (x3(SAMAUDIO_CLS_QKV)) SA_TRY(reg_.need_twin(L + "wqkv.x3", 3 * W, 3L * W, w.wqkv));
    if (x3(SAMAUDIO_CLS_WO)) SA_TRY(reg_.need_twin(L + "wo.x3", W, 3L * W, w.wo));
    if (x3(SAMAUDIO_CLS_W13)) SA_TRY(reg_.need_twin(L + "w1.x3", F, 3L * W, w.w1));
    if (x3(SAMAUDIO_CLS_W2)) SA_TRY(reg_.need_twin(L + "w2.x3", W, 3L * F, w.w2));
  }
  if (c.pool_type == 2) {
    NEEDF(reg_, g_.pool_q, "pool.q", W);             // in_proj_q(probe): the same query for every frame
    NEEDW(reg_, AT, g_.pool_wkv.w, "pool.wkv", 2 * W, W); NEEDF(reg_, g_.pool_bkv, "pool.bkv", 2 * W);
    if (x3(SAMAUDIO_CLS_QKV)) SA_TRY(reg_.need_twin("pool.wkv.x3", 2 * W, 3L * W, g_.pool_wkv));   // the same launch form on every token
    NEEDW(reg_, AT, g_.pool_wo, "pool.wo", W, W); NEEDF(reg_, g_.pool_bo, "pool.bo", W);
    NEEDF(reg_, g_.pool_ln_w, "pool.ln.w", W); NEEDF(reg_, g_.pool_ln_b, "pool.ln.b", W);
    NEEDW(reg_, AT, g_.pool_w1, "pool.w1", F, W); NEEDF(reg_, g_.pool_b1, "pool.b1", F);
    NEEDW(reg_, AT, g_.pool_w2, "pool.w2", W, F); NEEDF(reg_, g_.pool_b2, "pool.b2", W);
  }
  NEEDW(reg_, AT, g_.proj, "proj", c.output_dim, W);     // proj^T (features = pooled @ proj)
  if (x3_ && W > 256 * 8) return fail(SAMAUDIO_ERR_ARG, "vision tower: SAMAUDIO_OPT_X3_CLASSES needs width <= 2048 (launch_layernorm_rows_split3)");
  ready_ = true;
  return Status{};
}

void VisionTower::plan(Bump& b, int n, bool assign) {
  const long W = cfg_.width, F = cfg_.mlp_width, H = cfg_.heads, S = tokens(), Sp = round_up(S, 128);
  const long M = (long)n * S;
  auto f32 = [&](long k) { return (float*)b.take((size_t)k * 4); };
  auto act = [&](long k) { return b.take((size_t)k * esz_); };
  float* h = f32(M * W);
  void* xn = act(M * W); void* qkv = act(M * 3 * W);
  void* Q = act((long)n * H * Sp * hd_); void* K = act((long)n * H * Sp * hd_); void* Vt = act((long)n * H * hd_ * Sp);
  void* attn = act(M * W);
  void* u = b.take((size_t)M * F * esz_ > (size_t)M * W * 4 ? (size_t)M * F * esz_ : (size_t)M * W * 4);  // also the pre-LN embedding (f32)
  void* patches = act((long)n * grid_ * grid_ * kp_);
  unsigned char* mask = (unsigned char*)b.take((size_t)M);
  void* kv = act(M * 2 * W); void* pooled = act((long)n * W); float* y = f32((long)n * W); void* yn = act((long)n * W);
  void* u2 = act((long)n * F); float* z = f32((long)n * W); void* z_act = act((long)n * W);
  // SAMAUDIO_OPT_X3_CLASSES: the split operands, 3 x 16 bits per element, only those a switched class reads.  x3a serves the W-wide
  // operands one after the other: the LayerNorm rows (QKV, W13, pool.wkv), then the attention's split output / the split of its fp32
  // output (WO) - each is consumed by the next launch; x3u is the MLP hidden (W2)
  const size_t x3a_bytes = x3(SAMAUDIO_CLS_QKV | SAMAUDIO_CLS_WO | SAMAUDIO_CLS_W13) ? (size_t)M * 3 * W * 2 : 0;
  const size_t x3u_bytes = x3(SAMAUDIO_CLS_W2) ? (size_t)M * 3 * F * 2 : 0;
  void* x3a = x3a_bytes ? b.take(x3a_bytes) : nullptr; void* x3u = x3u_bytes ? b.take(x3u_bytes) : nullptr;
  if (assign) {
    w_.x3a = x3a; w_.x3u = x3u; w_.x3a_bytes = x3a_bytes; w_.x3u_bytes = x3u_bytes;
    w_.h = h; w_.xn = xn; w_.qkv = qkv; w_.Q = Q; w_.K = K; w_.Vt = Vt; w_.attn = attn; w_.u = u; w_.patches = patches;
    w_.mask = mask; w_.kv = kv; w_.pooled = pooled; w_.y = y; w_.yn = yn; w_.u2 = u2; w_.z = z; w_.z_act = z_act;
  }
}

size_t VisionTower::workspace_bytes(int n) {
  if (n <= 0) return 0;
  Bump b;
  plan(b, n, false);
  return b.used();
}

Status VisionTower::set_workspace(void* p, size_t bytes) {
  if (!p || (reinterpret_cast<uintptr_t>(p) & 255)) return fail(SAMAUDIO_ERR_WORKSPACE, "vision tower: workspace must be 256-byte aligned");
  ws_ = (char*)p;
  ws_bytes_ = bytes;
  planned_n_ = 0;
  return Status{};
}

Status VisionTower::prepare(const void* frames, const float* features, int n) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, "vision tower: weights not finalized");
  if (!frames || !features || n <= 0) return fail(SAMAUDIO_ERR_ARG, "vision tower: bad argument");
  if (!ws_) return fail(SAMAUDIO_ERR_WORKSPACE, "vision tower: no workspace");
  if (planned_n_ != n) {
    Bump b(ws_, ws_bytes_);
    plan(b, n, true);
    if (!b.fits()) return fail(SAMAUDIO_ERR_WORKSPACE, "vision tower: workspace too small for " + std::to_string(n) + " frames");
    planned_n_ = n;
  }
  return Status{};
}

// im2col rows of frames the caller has resized and normalised
Status VisionTower::encode(const float* frames, int n, bool normalize, float* features, float* tokens_out, hipStream_t st) {
  SA_TRY(prepare(frames, features, n));
  SA_HIP(launch_patchify(frames, w_.patches, bf16_, n, cfg_.image_size, cfg_.patch_size, kp_, st));
  return encode_patches(n, normalize, features, tokens_out, st);
}

// ... of raw uint8 frames: resize, rounding and normalisation in the launch that writes the rows
Status VisionTower::encode_frames(const uint8_t* frames, int n, int height, int width, int mode, bool normalize, float* features,
                                  float* tokens_out, hipStream_t st) {
  if (height < 1 || width < 1) return fail(SAMAUDIO_ERR_ARG, "vision tower: frame height / width < 1");
  if (mode != SAMAUDIO_RESIZE_NEAREST && mode != SAMAUDIO_RESIZE_BILINEAR && mode != SAMAUDIO_RESIZE_BICUBIC)
    return fail(SAMAUDIO_ERR_ARG, "vision tower: unknown resize mode");
  SA_TRY(prepare(frames, features, n));
  SA_HIP(launch_resize_frames(frames, n, height, width, cfg_.image_size, mode, w_.patches, bf16_, cfg_.patch_size, kp_, st));
  return encode_patches(n, normalize, features, tokens_out, st);
}

// ... of frames picked from a raw uint8 video, masked on the way: the same launch with an index table and a mask
Status VisionTower::encode_video(const uint8_t* frames, int64_t src_frames, int height, int width, const uint8_t* mask,
                                 int mask_channels, const int32_t* pick, int n, int mode, bool normalize, float* features,
                                 float* tokens_out, hipStream_t st) {
  if (!frames || !features || src_frames < 1 || src_frames > INT32_MAX || n < 1 || height < 1 || width < 1)
    return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_encode_video: null argument / src_frames, n, height, width < 1");
  if (mask && mask_channels != 1 && mask_channels != 3)
    return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_encode_video: mask_channels must be 1 or 3");
  if (mode != SAMAUDIO_RESIZE_NEAREST && mode != SAMAUDIO_RESIZE_BILINEAR && mode != SAMAUDIO_RESIZE_BICUBIC)
    return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_encode_video: unknown resize mode");
  if (!pick && n != src_frames) return fail(SAMAUDIO_ERR_ARG, "samaudio_vit_encode_video: no pick table, but n != src_frames");
  if (!launch_resize_video) return fail(SAMAUDIO_ERR_STATE, "samaudio_vit_encode_video: not in this build of the library");
  SA_TRY(prepare(frames, features, n));
  SA_HIP(launch_resize_video(frames, (long)src_frames, height, width, mask, mask_channels, pick, n, cfg_.image_size, mode, w_.patches,
                             bf16_, cfg_.patch_size, kp_, st));
  return encode_patches(n, normalize, features, tokens_out, st);
}

Status VisionTower::encode_patches(int n, bool normalize, float* features, float* tokens_out, hipStream_t st) {
  const samaudio_vit_config& c = cfg_;
  const int W = c.width, F = c.mlp_width, H = c.heads, S = tokens(), Sp = (int)round_up(S, 128), G2 = grid_ * grid_;
  const int cls = c.use_cls_token ? 1 : 0;
  const long M = (long)n * S;
  const float eps = c.ln_eps;
  float* emb = c.use_ln_pre ? (float*)w_.u : w_.h;  // the pre-LN embedding lives in the (still unused) MLP scratch

  // patch embedding: conv1 (k = stride = P, no bias) as one GEMM per frame over the im2col rows in w_.patches, + position rows 1..   (oracle: conv2d, + positional_embedding)
  {
    GemmParams p = lin(w_.patches, kp_, g_.patch_w, G2, W, kp_);
    p.nbatch = n; p.a_bstride = (long)G2 * kp_;
    p.res = g_.pos; p.res_ld = W; p.res_off = (long)cls * W; p.res_bstride = 0;
    p.out_f32 = emb; p.f32_ld = W; p.f32_bstride = (long)S * W; p.f32_off = (long)cls * W;
    SA_TRY(run_gemm(p, bf16_, kWho, st));
  }
  // class-token row (= class_embedding + positional_embedding[0], folded at load) and the all-valid key mask
  if (cls) {
    SA_HIP(launch_peav_cls_mask(emb, g_.pos, nullptr, w_.mask, n, S - 1, W, st));
  } else {
    SA_HIP(hipMemsetAsync(w_.mask, 1, (size_t)M, st));
  }
  if (c.use_ln_pre) SA_HIP(launch_layernorm_rows(emb, W, g_.ln_pre_w, g_.ln_pre_b, w_.h, nullptr, bf16_, M, W, eps, st));

  // LayerNorm in front of a GEMM: the GEMM-operand rows into xn, or - the GEMM's class on compensated operands - the split rows
  // [lo | hi | hi] into x3a in the same launch
  auto norm = [&](const float* x, const float* lw, const float* lb, bool split) -> Status {
    if (!split) {
      SA_HIP(launch_layernorm_rows(x, W, lw, lb, nullptr, w_.xn, bf16_, M, W, eps, st));
      return Status{};
    }
    SA_TRY(x3_fits(w_.x3a, w_.x3a_bytes, M, W, "vision tower: ", "the split LayerNorm rows do not fit the workspace plan"));
    SA_HIP(launch_layernorm_rows_split3(x, W, lw, lb, w_.x3a, M, W, eps, st));
    return Status{};
  };
  const bool qkv3 = x3(SAMAUDIO_CLS_QKV), wo3 = x3(SAMAUDIO_CLS_WO), w13_3 = x3(SAMAUDIO_CLS_W13), w2_3 = x3(SAMAUDIO_CLS_W2),
             att3 = x3(SAMAUDIO_X3_ATTENTION);
  for (int l = 0; l < c.layers; ++l) {  // oracle: resblocks
    const LayerW& w = layers_[l];
    SA_TRY(norm(w_.h, w.ln1_w, w.ln1_b, qkv3));
    {
      GemmParams p = lin(w_.xn, W, nullptr, M, 3 * W, W);   // (W: linear sets it from the record, here and below)
      p.bias = w.bqkv;
      p.out_act = w_.qkv; p.act_ld = 3L * W;
      SA_TRY(linear(p, w.wqkv, SAMAUDIO_CLS_QKV, X3Operand{w_.x3a, nullptr, 0}, st));
    }
    SA_HIP(launch_rope2d_split(w_.qkv, g_.rope_cos, g_.rope_sin, w_.Q, w_.K, w_.Vt, bf16_, n, S, Sp, H, hd_, st));
    const void* attn_split = nullptr;   // the context rows in split form, when the attention wrote them for wo
    if (att3) {   // fp32 tensors, both contractions on hi/lo-split operands (Sp % 128 == 0)
      if (wo3) SA_TRY(x3_fits(w_.x3a, w_.x3a_bytes, M, W, "vision tower: ", "the attention's split output does not fit the workspace plan"));
      SA_HIP(launch_self_attention_x3((const float*)w_.Q, (const float*)w_.K, (const float*)w_.Vt, w_.mask, (float*)w_.attn, n, S, Sp, H,
                                      hd_, st, wo3 ? w_.x3a : nullptr));
      if (wo3) attn_split = w_.x3a;
    } else {
      SA_HIP(launch_self_attention_hd(w_.Q, w_.K, w_.Vt, w_.mask, w_.attn, bf16_, n, S, Sp, H, hd_, st));
    }
    {
      GemmParams p = lin(w_.attn, W, nullptr, M, W, W);  // x = x + out_proj(attn)
      p.bias = w.bo;
      p.res = w_.h; p.res_ld = W;
      p.out_f32 = w_.h; p.f32_ld = W;
      SA_TRY(linear(p, w.wo, SAMAUDIO_CLS_WO, X3Operand{attn_split, w_.x3a, w_.x3a_bytes}, st));
    }
    SA_TRY(norm(w_.h, w.ln2_w, w.ln2_b, w13_3));
    {
      GemmParams p = lin(w_.xn, W, nullptr, M, F, W);  // act(c_fc(x))
      p.bias = w.b1; p.act = c.act;
      p.out_act = w_.u; p.act_ld = F;
      // c_fc writes c_proj's operand in split form where the launch it would make passes gemm_check (the register epilogue of the
      // 8-phase family: bias + GELU with a split output); otherwise fp32 output + launch_split3 in front of c_proj
      const bool w2_pre = w13_3 && w2_3 && x3_w2_pre(p, w_.x3a, w.w1, w_.x3u, w_.x3u_bytes, M, F, [](const GemmParams& q) {
        return x3_share(q, SAMAUDIO_CLS_W13);
      });
      if (w2_pre) { p.out_act = w_.x3u; p.flags |= GEMM_FLAG_OUT_SPLIT3; }
      SA_TRY(linear(p, w.w1, SAMAUDIO_CLS_W13, X3Operand{w_.x3a, nullptr, 0}, st));
      p = lin(w_.u, F, nullptr, M, W, F);  // x = x + c_proj(...)
      p.bias = w.b2;
      p.res = w_.h; p.res_ld = W;
      p.out_f32 = w_.h; p.f32_ld = W;
      SA_TRY(linear(p, w.w2, SAMAUDIO_CLS_W2, X3Operand{w2_pre ? w_.x3u : nullptr, w_.x3u, w_.x3u_bytes}, st));
    }
  }
  if (tokens_out) SA_HIP(hipMemcpyAsync(tokens_out, w_.h, (size_t)M * W * 4, hipMemcpyDeviceToDevice, st));

  // ln_post on every token, then pooling                                                   (oracle: ln_post, _pool)
  const void* pooled_act = nullptr;  // [n, W] GEMM operand of the projection
  if (c.pool_type == 2) {
    const void* kv_split = nullptr;   // class QKV: ln_post writes the split rows; without ln_post, linear splits h itself
    if (c.use_ln_post) {
      SA_TRY(norm(w_.h, g_.ln_post_w, g_.ln_post_b, qkv3));
      if (qkv3) kv_split = w_.x3a;
    } else if (!qkv3) {
      SA_HIP(launch_to_act(w_.h, 0, W, 0, w_.xn, 0, bf16_, 1, M, W, W, 0, st));
    }
    {
      GemmParams p = lin(qkv3 && !c.use_ln_post ? (const void*)w_.h : w_.xn, W, nullptr, M, 2 * W, W);  // k | v of every token
      p.bias = g_.pool_bkv;
      p.out_act = w_.kv; p.act_ld = 2L * W;
      SA_TRY(linear(p, g_.pool_wkv, SAMAUDIO_CLS_QKV, X3Operand{kv_split, w_.x3a, w_.x3a_bytes}, st));
    }
    SA_HIP(launch_pool_attention(g_.pool_q, w_.kv, w_.pooled, bf16_, n, S, c.pool_heads, pool_hd_, st));
    {
      GemmParams p = lin(w_.pooled, W, g_.pool_wo, n, W, W);  // y = out_proj(attention)
      p.bias = g_.pool_bo;
      p.out_f32 = w_.y; p.f32_ld = W;
      SA_TRY(run_gemm(p, bf16_, kWho, st));
    }
    SA_HIP(launch_layernorm_rows(w_.y, W, g_.pool_ln_w, g_.pool_ln_b, nullptr, w_.yn, bf16_, n, W, eps, st));
    {
      GemmParams p = lin(w_.yn, W, g_.pool_w1, n, F, W);
      p.bias = g_.pool_b1; p.act = c.act;
      p.out_act = w_.u2; p.act_ld = F;
      SA_TRY(run_gemm(p, bf16_, kWho, st));
      p = lin(w_.u2, F, g_.pool_w2, n, W, F);  // z = y + mlp(layernorm(y))
      p.bias = g_.pool_b2;
      p.res = w_.y; p.res_ld = W;
      p.out_f32 = w_.z; p.f32_ld = W;
      p.out_act = w_.z_act; p.act_ld = W;
      SA_TRY(run_gemm(p, bf16_, kWho, st));
    }
    pooled_act = w_.z_act;
  } else if (c.pool_type == 0) {
    // class token: LayerNorm of row 0 of every frame (rows are S*W apart)
    if (c.use_ln_post) SA_HIP(launch_layernorm_rows(w_.h, (long)S * W, g_.ln_post_w, g_.ln_post_b, nullptr, w_.z_act, bf16_, n, W, eps, st));
    else SA_HIP(launch_to_act(w_.h, 0, (long)S * W, 0, w_.z_act, 0, bf16_, 1, n, W, W, 0, st));
    pooled_act = w_.z_act;
  } else {
    float* src = w_.h;
    if (c.use_ln_post) {
      SA_HIP(launch_layernorm_rows(w_.h, W, g_.ln_post_w, g_.ln_post_b, (float*)w_.u, nullptr, bf16_, M, W, eps, st));
      src = (float*)w_.u;
    }
    SA_HIP(launch_token_mean(src, W, nullptr, w_.z_act, bf16_, n, S, W, st));
    pooled_act = w_.z_act;
  }
  {
    GemmParams p = lin(pooled_act, W, g_.proj, n, c.output_dim, W);  // features = pooled @ proj
    p.out_f32 = features; p.f32_ld = c.output_dim;
    SA_TRY(run_gemm(p, bf16_, kWho, st));
  }
  if (normalize) SA_HIP(launch_l2_normalize(features, n, c.output_dim, st));
  return Status{};
}

}  // namespace sa

extern "C" {

int samaudio_vit_create(const samaudio_vit_config* cfg, samaudio_vit** out) {
  if (!cfg || !out) return sa::bad("samaudio_vit_create: null argument");
  if (cfg->precision != SAMAUDIO_F32 && cfg->precision != SAMAUDIO_BF16) return sa::bad("samaudio_vit_create: precision");
  samaudio_vit* v = new samaudio_vit;
  v->tower = new sa::VisionTower(*cfg);
  *out = v;
  return SAMAUDIO_OK;
}

void samaudio_vit_destroy(samaudio_vit* v) {
  if (!v) return;
  delete v->tower;
  delete v;
}

int samaudio_vit_set_tensor(samaudio_vit* v, const char* name, const void* data, int dtype, int ndim, const int64_t* shape) {
  return SA_ENTRY(v, "null vision tower", v->tower->set_tensor(name, data, dtype, ndim, shape));
}

int samaudio_vit_set_option(samaudio_vit* v, int option, int value) {
  return SA_ENTRY(v, "null vision tower", v->tower->set_option(option, value));
}

int samaudio_vit_finalize(samaudio_vit* v) {
  return SA_ENTRY(v, "null vision tower", v->tower->finalize());
}

size_t samaudio_vit_workspace_bytes(samaudio_vit* v, int frames) {
  if (!v) return 0;
  return v->tower->workspace_bytes(frames);
}

int samaudio_vit_set_workspace(samaudio_vit* v, void* workspace, size_t bytes) {
  return SA_ENTRY(v, "null vision tower", v->tower->set_workspace(workspace, bytes));
}

int samaudio_vit_encode(samaudio_vit* v, const float* frames, int n, int normalize, float* features, float* tokens_out,
                        samaudio_stream stream) {
  return SA_ENTRY(v, "null vision tower", v->tower->encode(frames, n, normalize != 0, features, tokens_out, (hipStream_t)stream));
}

int samaudio_vit_encode_frames(samaudio_vit* v, const uint8_t* frames, int n, int height, int width, int mode, int normalize,
                               float* features, float* tokens_out, samaudio_stream stream) {
  return SA_ENTRY(v, "null vision tower",
                  v->tower->encode_frames(frames, n, height, width, mode, normalize != 0, features, tokens_out,
                      (hipStream_t)stream));
}

int samaudio_vit_encode_video(samaudio_vit* v, const uint8_t* frames, int64_t src_frames, int height, int width, const uint8_t* mask,
                              int mask_channels, const int32_t* pick, int n, int mode, int normalize, float* features,
                              float* tokens_out, samaudio_stream stream) {
  return SA_ENTRY(v, "samaudio_vit_encode_video: null vision tower",
                  v->tower->encode_video(frames, src_frames, height, width, mask, mask_channels, pick, n, mode, normalize != 0,
                      features, tokens_out, (hipStream_t)stream));
}

}  // extern "C"
