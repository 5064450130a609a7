// PE-AV transformer, Judge glue and PE-A-Frame logits: host code that sequences kernels of gemm*.hip / kernels.hip /
// attention.hip / peav_kernels.hip.  "hf:" = transformers/models/pe_audio/modeling_pe_audio.py (the Hugging Face port
// of the un-vendored perception_models network, see peav.h); "judge.py" = reference sam_audio/model/judge.py.
#include "peav.h"

#include <cstring>

namespace sa {

namespace {
Status check_dims(const samaudio_peav_dims& d, const char* who) {
  if (d.dim <= 0 || d.n_heads <= 0 || d.n_layers < 0 || d.ffn_hidden <= 0 || d.in_dim <= 0 || d.max_positions <= 0)
    return fail(SAMAUDIO_ERR_ARG, std::string(who) + ": non-positive dimension");
  if (d.n_heads * 128 != d.dim || d.dim % 256)
    return fail(SAMAUDIO_ERR_ARG, std::string(who) + ": dim must be n_heads * 128 and a multiple of 256");
  if ( d.ffn_hidden % 64 || d.in_dim % 64)
    return fail(SAMAUDIO_ERR_ARG, std::string(who) + ": widths must be multiples of 64");
  return Status{};
}
}  // namespace

// ---------------------------------------------------------------------------------------------------
// PE-AV transformer
// ---------------------------------------------------------------------------------------------------
PeavEncoder::PeavEncoder(const samaudio_peav_dims& d, bool bf16, std::string prefix)
    : d_(d), bf16_(bf16), esz_(bf16 ? 2 : 4), prefix_(std::move(prefix)), who_(prefix_ + ": ") {}

Status PeavEncoder::finalize(const Registry& reg) {
  SA_TRY(check_dims(d_, prefix_.c_str()));
  const int D = d_.dim, F = d_.ffn_hidden;
  const int AT = bf16_ ? SAMAUDIO_DT_BF16 : SAMAUDIO_DT_F32;
  const std::string& P = prefix_;
  NEEDW(reg, AT, g_.in_w, P + "in.w", D, d_.in_dim);
  NEEDF(reg, g_.in_b, P + "in.b", D);
  NEEDF(reg, g_.cls, P + "cls", D);
  NEEDF(reg, g_.gn1_w, P + "gn1.w", D);
  NEEDF(reg, g_.gn1_b, P + "gn1.b", D);
  NEEDW(reg, AT, g_.conv1.w, P + "conv1.w", D, 3 * D);
  NEEDF(reg, g_.conv1_b, P + "conv1.b", D);
  NEEDF(reg, g_.gn2_w, P + "gn2.w", D);
  NEEDF(reg, g_.gn2_b, P + "gn2.b", D);
  NEEDW(reg, AT, g_.conv2.w, P + "conv2.w", D, 3 * D);
  NEEDF(reg, g_.conv2_b, P + "conv2.b", D);
  NEEDF(reg, g_.norm, P + "norm", D);
  NEEDW(reg, AT, g_.out.w, P + "out.w", D, D);
  NEEDF(reg, g_.rope_cos, P + "rope_cos", d_.max_positions, 64);
  NEEDF(reg, g_.rope_sin, P + "rope_sin", d_.max_positions, 64);
  layers_.assign(d_.n_layers, LayerW{});
  for (int i = 0; i < d_.n_layers; ++i) {
    const std::string L = P + "L" + std::to_string(i) + ".";
    LayerW& w = layers_[i];
    NEEDF(reg, w.attn_norm, L + "attn_norm", D);
    NEEDF(reg, w.ffn_norm, L + "ffn_norm", D);
    NEEDF(reg, w.q_norm, L + "q_norm", 128);
    NEEDF(reg, w.k_norm, L + "k_norm", 128);
    NEEDW(reg, AT, w.wqkv.w, L + "wqkv", 3 * D, D);
    NEEDW(reg, AT, w.wo.w, L + "wo", D, D);
    NEEDW(reg, AT, w.w13.w, L + "w13", 2 * F, D);
    NEEDW(reg, AT, w.w2.w, L + "w2", D, F);
    w.bqkv = w.bo = nullptr;
    if (d_.attn_bias) {
      NEEDF(reg, w.bqkv, L + "bqkv", 3 * D);
      NEEDF(reg, w.bo, L + "bo", D);
    }
    // SAMAUDIO_OPT_X3_CLASSES: the twins of the classes that are switched on, and the [gain | 0] tables of the norms in front of them
    if (x3(SAMAUDIO_CLS_QKV)) {
      SA_TRY(reg.need_twin(L + "wqkv.x3", 3 * D, 3L * D, w.wqkv));
      NEEDF(reg, w.attn_gs, L + "attn_norm.gs", 2, D);
    }
    if (x3(SAMAUDIO_CLS_WO)) SA_TRY(reg.need_twin(L + "wo.x3", D, 3L * D, w.wo));
    if (x3(SAMAUDIO_CLS_W13)) {
      SA_TRY(reg.need_twin(L + "w13.x3", 2 * F, 3L * D, w.w13));
      NEEDF(reg, w.ffn_gs, L + "ffn_norm.gs", 2, D);
    }
    if (x3(SAMAUDIO_CLS_W2)) SA_TRY(reg.need_twin(L + "w2.x3", D, 3L * F, w.w2));
  }
  if (x3(SAMAUDIO_CLS_PATCH)) {
    SA_TRY(reg.need_twin(P + "conv1.w.x3", D, 9L * D, g_.conv1));
    SA_TRY(reg.need_twin(P + "conv2.w.x3", D, 9L * D, g_.conv2));
  }
  if (x3(SAMAUDIO_CLS_WO)) {
    SA_TRY(reg.need_twin(P + "out.w.x3", D, 3L * D, g_.out));
    NEEDF(reg, g_.norm_gs, P + "norm.gs", 2, D);
  }
  if (x3_ && D > 256 * 12) return fail(SAMAUDIO_ERR_ARG, P + ": SAMAUDIO_OPT_X3_CLASSES needs dim <= 3072 (launch_rmsnorm_gs_split3)");
  ready_ = true;
  return Status{};
}

void PeavEncoder::plan(Bump& b, int rows, int frames, bool assign) {
  const long D = d_.dim, F = d_.ffn_hidden, H = d_.n_heads, S = frames + 1, Sp = round_up(S, 64);
  const long M = (long)rows * S;
  auto f32 = [&](long n) { return (float*)b.take((size_t)n * 4); };
  auto act = [&](long n) { return b.take((size_t)n * esz_); };
  float* h0 = f32(M * D); float* r1 = f32(M * D); float* h = f32(M * D); float* out = f32(M * D);
  void* out_act = act(M * D); void* xn = act(M * D); void* qkv = act(M * 3 * D);
  void* Q = act((long)rows * H * Sp * 128); void* K = act((long)rows * H * Sp * 128);
  void* Vt = act((long)rows * H * 128 * Sp);
  void* attn = act(M * D); void* u = act(M * F); void* gnbuf = act((long)rows * (S + 2) * D);
  unsigned char* mask_s = (unsigned char*)b.take((size_t)M);
  double* gn_part = (double*)b.take((size_t)rows * 64 * 3 * 8);
  // SAMAUDIO_OPT_X3_CLASSES: the split operands, 3 x 16 bits per element, only those a switched class reads
  const bool gemms = x3(SAMAUDIO_CLS_QKV | SAMAUDIO_CLS_WO | SAMAUDIO_CLS_W13 | SAMAUDIO_CLS_W2);
  const size_t x3a_bytes = gemms ? (size_t)M * 3 * D * 2 : 0, x3u_bytes = x3(SAMAUDIO_CLS_W2) ? (size_t)M * 3 * F * 2 : 0;
  const size_t gn3_bytes = x3(SAMAUDIO_CLS_PATCH) ? (size_t)rows * (S + 2) * 3 * D * 2 : 0;
  const size_t attn3_bytes = x3(SAMAUDIO_CLS_WO) && x3(SAMAUDIO_X3_ATTENTION) ? (size_t)M * 3 * D * 2 : 0;
  void* x3a = x3a_bytes ? b.take(x3a_bytes) : nullptr; void* x3u = x3u_bytes ? b.take(x3u_bytes) : nullptr;
  void* gn3 = gn3_bytes ? b.take(gn3_bytes) : nullptr; void* attn3 = attn3_bytes ? b.take(attn3_bytes) : nullptr;
  if (assign) {
    w_.x3a = x3a; w_.x3u = x3u; w_.gn3 = gn3; w_.attn3 = attn3;
    w_.x3a_bytes = x3a_bytes; w_.x3u_bytes = x3u_bytes; w_.gn3_bytes = gn3_bytes; w_.attn3_bytes = attn3_bytes;
    w_.h0 = h0; w_.r1 = r1; w_.h = h; w_.out = out; w_.out_act = out_act; w_.xn = xn; w_.qkv = qkv; w_.Q = Q; w_.K = K;
    w_.Vt = Vt; w_.attn = attn; w_.u = u; w_.gnbuf = gnbuf; w_.mask_s = mask_s; w_.gn_part = gn_part;
  }
}

Status PeavEncoder::forward(const void* x_act, const unsigned char* pad_mask, int rows, int T, hipStream_t st) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, prefix_ + ": weights not finalized");
  if (!x_act || rows <= 0 || T <= 0) return fail(SAMAUDIO_ERR_ARG, prefix_ + ": bad shape");
  if (T + 1 > d_.max_positions) return fail(SAMAUDIO_ERR_ARG, prefix_ + ": more frames than RoPE positions");
  if (!w_.h0) return fail(SAMAUDIO_ERR_WORKSPACE, prefix_ + ": workspace not planned");
  const int D = d_.dim, F = d_.ffn_hidden, H = d_.n_heads, S = T + 1, Sp = (int)round_up(S, 64);
  const long M = (long)rows * S;
  const float eps = d_.norm_eps;

  // h0[b][1 + t] = in_proj(x[b][t])   (judge.py:109 data_proj / :124-126 finetune_data_proj; hf:174 data_proj)
  {
    GemmParams p = lin(x_act, d_.in_dim, g_.in_w, T, D, d_.in_dim);
    p.nbatch = rows; p.a_bstride = (long)T * d_.in_dim; p.bias = g_.in_b;
    p.out_f32 = w_.h0; p.f32_bstride = (long)S * D; p.f32_ld = D; p.f32_off = D;
    SA_TRY(run_gemm(p, bf16_, "", st));
  }
  // class token + sequence mask                                                    (hf:273-285)
  SA_HIP(launch_peav_cls_mask(w_.h0, g_.cls, pad_mask, w_.mask_s, rows, T, D, st));
  // ResNet block: h = h0 + conv(silu(mgn(conv(silu(mgn(h0))))))                     (hf:224-263)
  const bool patch3 = x3(SAMAUDIO_CLS_PATCH);
  // (weak launcher: absent in a library linked against the CPU emulation of the launchers - fp32 buffer + launch_split3 then)
  const bool gn_direct = patch3 && launch_masked_groupnorm_silu_split3 != nullptr;
  if (patch3) SA_TRY(x3_fits(w_.gn3, w_.gn3_bytes, (long)rows * (S + 2), D, prefix_ + ": ", "the split halo buffer does not fit the workspace plan"));
  // zero halo rows = 'same' padding (the split form of a zero row is a zero row)
  if (gn_direct) SA_HIP(hipMemsetAsync(w_.gn3, 0, (size_t)rows * (S + 2) * 3 * D * 2, st));
  else SA_HIP(hipMemsetAsync(w_.gnbuf, 0, (size_t)rows * (S + 2) * D * esz_, st));
  auto gn_silu = [&](const float* x, const float* gw, const float* gb) -> Status {
    if (gn_direct) {
      SA_HIP(launch_masked_groupnorm_silu_split3(x, gw, gb, w_.mask_s, w_.gn_part, w_.gn3, rows, S, D, 1, 1e-5f, st));
      return Status{};
    }
    SA_HIP(launch_masked_groupnorm_silu(x, gw, gb, w_.mask_s, w_.gn_part, w_.gnbuf, bf16_, rows, S, D, 1, 1e-5f, st));
    if (patch3) SA_HIP(launch_split3((const float*)w_.gnbuf, D, w_.gn3, (long)rows * (S + 2), D, st));
    return Status{};
  };
  // (compensated operands: a tap of the convolution is 3 D contiguous elements [lo | hi | hi] of a halo-buffer row of gn3 against that
  // tap's [W_hi | W_lo | W_hi])
  auto conv3 = [&](const LinW& w, const float* bias, const float* skip, float* dst) -> Status {
    GemmParams p = lin(w_.gnbuf, D, nullptr, S, D, 3 * D);
    p.kc = D; p.tap_stride = D; p.a_bstride = (long)(S + 2) * D; p.nbatch = rows; p.bias = bias;
    if (skip) { p.res = skip; p.res_ld = D; p.res_bstride = (long)S * D; }
    p.out_f32 = dst; p.f32_ld = D; p.f32_bstride = (long)S * D;
    return linear(p, w, SAMAUDIO_CLS_PATCH, X3Operand{w_.gn3, nullptr, 0, true}, st);
  };
  SA_TRY(gn_silu(w_.h0, g_.gn1_w, g_.gn1_b));
  SA_TRY(conv3(g_.conv1, g_.conv1_b, nullptr, w_.r1));
  SA_TRY(gn_silu(w_.r1, g_.gn2_w, g_.gn2_b));
  SA_TRY(conv3(g_.conv2, g_.conv2_b, w_.h0, w_.h));

  // RMSNorm in front of a GEMM: fp32 rows into xn, or - the GEMM's class on compensated operands - the split rows into x3a
  auto norm = [&](const float* w, const float* gs, bool split) -> Status {
    if (!split) {
      SA_HIP(launch_rmsnorm_mod(w_.h, w, nullptr, nullptr, nullptr, 0, 0, 0, w_.xn, bf16_, (int)M, D, S, eps, st));
      return Status{};
    }
    SA_TRY(x3_fits(w_.x3a, w_.x3a_bytes, M, D, prefix_ + ": ", "the split operand does not fit the workspace plan"));
    SA_HIP(launch_rmsnorm_gs_split3(w_.h, gs, 0, w_.x3a, (int)M, D, S, eps, st));
    return Status{};
  };
  const bool qkv3 = x3(SAMAUDIO_CLS_QKV), wo3 = x3(SAMAUDIO_CLS_WO), w13_3 = x3(SAMAUDIO_CLS_W13), w2_3 = x3(SAMAUDIO_CLS_W2),
             att3 = x3(SAMAUDIO_X3_ATTENTION);
  for (int l = 0; l < d_.n_layers; ++l) {  // hf:457-490
    const LayerW& w = layers_[l];
    SA_TRY(norm(w.attn_norm, w.attn_gs, qkv3));
    {
      GemmParams p = lin(w_.xn, D, nullptr, M, 3 * D, D);   // (W: linear sets it from the record, here and below)
      p.bias = w.bqkv;
      p.out_act = w_.qkv; p.act_ld = 3L * D;
      SA_TRY(linear(p, w.wqkv, SAMAUDIO_CLS_QKV, X3Operand{w_.x3a, nullptr, 0}, st));
    }
    const void* attn_split = nullptr;   // the context rows in split form, when the attention wrote them for wo
    if (att3) {   // fp32 tensors, both contractions on hi/lo-split operands (head width 128, Sp % 64 == 0)
      if (wo3) SA_TRY(x3_fits(w_.attn3, w_.attn3_bytes, M, D, prefix_ + ": ", "the attention's split output does not fit the workspace plan"));
      SA_HIP(launch_qkv_prep_f32x((const float*)w_.qkv, w.q_norm, w.k_norm, g_.rope_cos, g_.rope_sin, (float*)w_.Q, (float*)w_.K,
                                  (float*)w_.Vt, rows, S, Sp, H, eps, st));
      SA_HIP(launch_self_attention_x3((const float*)w_.Q, (const float*)w_.K, (const float*)w_.Vt, w_.mask_s, (float*)w_.attn, rows, S,
                                      Sp, H, 128, st, wo3 ? w_.attn3 : nullptr));
      if (wo3) attn_split = w_.attn3;
    } else {
      SA_HIP(launch_qkv_prep(w_.qkv, w.q_norm, w.k_norm, g_.rope_cos, g_.rope_sin, w_.Q, w_.K, w_.Vt, bf16_, rows, S, Sp, H,
                             eps, st));
      SA_HIP(launch_self_attention(w_.Q, w_.K, w_.Vt, w_.mask_s, w_.attn, bf16_, rows, S, Sp, H, st));
    }
    {
      GemmParams p = lin(w_.attn, D, nullptr, M, D, D);  // h = h + o_proj(attn)
      p.bias = w.bo;
      p.res = w_.h; p.res_ld = D;
      p.out_f32 = w_.h; p.f32_ld = D;
      SA_TRY(linear(p, w.wo, SAMAUDIO_CLS_WO, X3Operand{attn_split, w_.x3a, w_.x3a_bytes}, st));
    }
    SA_TRY(norm(w.ffn_norm, w.ffn_gs, w13_3));
    {
      GemmParams p = lin(w_.xn, D, nullptr, M, 2 * F, D);
      p.swiglu = 1;
      p.out_act = w_.u; p.act_ld = F;
      // w13 writes w2's operand in split form where the launch it would make passes gemm_check
      const bool w2_pre = w13_3 && w2_3 && x3_w2_pre(p, w_.x3a, w.w13, w_.x3u, w_.x3u_bytes, M, F, [](const GemmParams& q) {
        return x3_share(q, SAMAUDIO_CLS_W13);
      });
      if (w2_pre) { p.out_act = w_.x3u; p.flags |= GEMM_FLAG_OUT_SPLIT3; }
      SA_TRY(linear(p, w.w13, SAMAUDIO_CLS_W13, X3Operand{w_.x3a, nullptr, 0}, st));
      p = lin(w_.u, F, nullptr, M, D, F);  // h = h + down_proj(...)
      p.res = w_.h; p.res_ld = D;
      p.out_f32 = w_.h; p.f32_ld = D;
      SA_TRY(linear(p, w.w2, SAMAUDIO_CLS_W2, X3Operand{w2_pre ? w_.x3u : nullptr, w_.x3u, w_.x3u_bytes}, st));
    }
  }
  // final norm + output projection                                                  (hf:672-673)
  SA_TRY(norm(g_.norm, g_.norm_gs, wo3));
  {
    GemmParams p = lin(w_.xn, D, nullptr, M, D, D);
    p.out_f32 = w_.out; p.f32_ld = D;
    // (x3: one output - the 16-bit operand copy of an fp32 context is the same fp32 tensor, out_act() in peav.h)
    if (!wo3) { p.out_act = w_.out_act; p.act_ld = D; }
    SA_TRY(linear(p, g_.out, SAMAUDIO_CLS_WO, X3Operand{w_.x3a, nullptr, 0}, st));
  }
  return Status{};
}

// ---------------------------------------------------------------------------------------------------
// Judge
// ---------------------------------------------------------------------------------------------------
static samaudio_peav_dims with_in_dim(samaudio_peav_dims d, int in_dim) {
  d.in_dim = in_dim;
  return d;
}

Judge::Judge(const samaudio_judge_config& c)
    : cfg_(c), bf16_(c.precision == SAMAUDIO_BF16), esz_(bf16_ ? 2 : 4),
      at_dtype_(bf16_ ? SAMAUDIO_DT_BF16 : SAMAUDIO_DT_F32),
      enc_(with_in_dim(c.transformer, c.codec_dim), bf16_, "t."),
      fin_(with_in_dim(c.finetune_transformer, c.bottleneck_dim), bf16_, "ft.") {}

Status Judge::set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape) {
  ready_ = false;
  return reg_.set(name, p, dtype, ndim, shape);
}

// SAMAUDIO_OPT_X3_CLASSES of a tower context (Judge / FramePredictor): fp32 contexts, tower bits only
static Status check_x3_option(int option, int value, bool bf16, const char* who) {
  if (option != SAMAUDIO_OPT_X3_CLASSES) return fail(SAMAUDIO_ERR_ARG, std::string(who) + ": unknown option");
  if (value && bf16)
    return fail(SAMAUDIO_ERR_ARG, std::string(who) + ": SAMAUDIO_OPT_X3_CLASSES applies to fp32 contexts (compensated 16-bit operands under fp32 storage)");
  if (value & ~SAMAUDIO_CLS_X3_TOWER)
    return fail(SAMAUDIO_ERR_ARG, std::string(who) + ": SAMAUDIO_OPT_X3_CLASSES: only qkv, wo, w13, w2, patch and SAMAUDIO_X3_ATTENTION");
  return Status{};
}

Status Judge::set_option(int option, int value) {
  SA_TRY(check_x3_option(option, value, bf16_, "samaudio_judge_set_option"));
  x3_ = value;
  enc_.set_x3(value);
  fin_.set_x3(value);
  ready_ = false;   // finalize resolves the twins of the switched classes
  return Status{};
}

Status Judge::finalize() {
  const int D = cfg_.transformer.dim, D2 = cfg_.finetune_transformer.dim, Bn = cfg_.bottleneck_dim,
            TH = cfg_.text_hidden;
  if (Bn <= 0 || Bn % 64 || TH <= 0 || TH % 64 || cfg_.codec_dim % 64)
    return fail(SAMAUDIO_ERR_ARG, "judge: bottleneck_dim / text_hidden / codec_dim must be positive multiples of 64");
  SA_TRY(enc_.finalize(reg_));
  SA_TRY(fin_.finalize(reg_));
  const int AT = at_dtype_;
  NEEDW(reg_, AT, g_.cat_wh.w, "cat.wh", Bn, D);     // cat_audio_proj.weight[:, :D]   (separated / hypothesis half, judge.py:113-115)
  NEEDW(reg_, AT, g_.cat_wi.w, "cat.wi", Bn, D);     // cat_audio_proj.weight[:, D:]   (mixture half)
  NEEDF(reg_, g_.cat_b, "cat.b", Bn);
  NEEDW(reg_, AT, g_.tp1_w, "tp1.w", D, TH);        // text_proj1 (no bias)
  NEEDW(reg_, AT, g_.tp2_w, "tp2.w", Bn, D);        // text_proj2
  NEEDF(reg_, g_.tp2_b, "tp2.b", Bn);
  NEEDF(reg_, g_.ln_w, "ln.w", Bn);
  NEEDF(reg_, g_.ln_b, "ln.b", Bn);
  NEEDW(reg_, AT, g_.pat_wa, "pat.wa", Bn, Bn);     // proj_audio_and_text.weight[:, :Bn]  (audio half, judge.py:121-123)
  NEEDW(reg_, AT, g_.pat_wt, "pat.wt", Bn, Bn);     // proj_audio_and_text.weight[:, Bn:]  (text half)
  NEEDF(reg_, g_.pat_b, "pat.b", Bn);
  NEEDF(reg_, g_.head_w, "head.w", 4, D2);
  NEEDF(reg_, g_.mean, "mean", 4);
  NEEDF(reg_, g_.std_, "std", 4);
  if (x3_ & SAMAUDIO_CLS_WO) {   // cat_audio_proj reads the transformer's output rows: K = D over all frames, with out.w's class
    SA_TRY(reg_.need_twin("cat.wh.x3", Bn, 3L * D, g_.cat_wh));
    SA_TRY(reg_.need_twin("cat.wi.x3", Bn, 3L * D, g_.cat_wi));
  }
  if (D2 > 4096) return fail(SAMAUDIO_ERR_ARG, "judge: finetune_transformer.dim > 4096");
  ready_ = true;
  return Status{};
}

void Judge::plan(Bump& b, int Bi, int cand, int T, bool assign) {
  const long Bp = (long)Bi * cand, N1 = Bi + Bp;
  const long D = cfg_.transformer.dim, Bn = cfg_.bottleneck_dim, CD = cfg_.codec_dim, TH = cfg_.text_hidden;
  auto f32 = [&](long n) { return (float*)b.take((size_t)n * 4); };
  auto act = [&](long n) { return b.take((size_t)n * esz_); };
  // long-lived across both transformer passes
  void* audio = act(Bp * T * Bn); void* at = act(Bp * T * Bn);
  void* tp_act = act(Bp * TH); void* t1 = act(Bp * D); void* tl = act(Bp * Bn);
  float* inp_part = f32((long)Bi * T * Bn); float* t2 = f32(Bp * Bn); float* tpart = f32(Bp * Bn);
  unsigned char* mask = (unsigned char*)b.take((size_t)N1 * T);
  void* xa = act(N1 * T * CD);
  if (assign) {
    w_.audio = audio; w_.at = at; w_.tp_act = tp_act; w_.t1 = t1; w_.tl = tl; w_.inp_part = inp_part; w_.t2 = t2;
    w_.tpart = tpart; w_.mask = mask; w_.xa = xa;
  }
  // the two transformers run one after the other and share the rest of the workspace
  const size_t mark = b.mark();
  enc_.plan(b, (int)N1, T, assign);
  const size_t used1 = b.mark();
  b.reset_to(mark);
  fin_.plan(b, (int)Bp, T, assign);
  if (b.mark() < used1) b.reset_to(used1);
}

size_t Judge::workspace_bytes(int inputs, int candidates, int frames) {
  if (inputs <= 0 || candidates <= 0 || frames <= 0) return 0;
  Bump b;
  plan(b, inputs, candidates, frames, false);
  return b.used() + 4096;
}

Status Judge::set_workspace(void* p, size_t bytes) {
  if (!p || (reinterpret_cast<uintptr_t>(p) & 255)) return fail(SAMAUDIO_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  ws_ = (char*)p;
  ws_bytes_ = bytes;
  return Status{};
}

Status Judge::score(const float* in_lat, const float* sep_lat, int Bi, int cand, int T, const float* text_pooled,
                    const unsigned char* pad_mask, float* scores, hipStream_t st) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, "judge_score: weights not finalized");
  if (!in_lat || !sep_lat || !text_pooled || !scores || Bi <= 0 || cand <= 0 || T <= 0)
    return fail(SAMAUDIO_ERR_ARG, "judge_score: bad argument");
  Bump b(ws_, ws_bytes_);
  plan(b, Bi, cand, T, true);
  if (!ws_ || !b.fits())
    return fail(SAMAUDIO_ERR_WORKSPACE, "judge_score: workspace too small (" + std::to_string(b.used()) + " bytes needed)");
  const int Bp = Bi * cand, N1 = Bi + Bp, S = T + 1;
  const int D = cfg_.transformer.dim, Bn = cfg_.bottleneck_dim, CD = cfg_.codec_dim, TH = cfg_.text_hidden,
            D2 = cfg_.finetune_transformer.dim;

  // stacked codec features [mixtures ; separations] and their frame masks             (judge.py:101-107)
  SA_HIP(launch_to_act(in_lat, 0, CD, 0, w_.xa, 0, bf16_, 1, (long)Bi * T, CD, CD, 0, st));
  SA_HIP(launch_to_act(sep_lat, 0, CD, 0, (char*)w_.xa + (size_t)Bi * T * CD * esz_, 0, bf16_, 1, (long)Bp * T, CD, CD, 0, st));
  const unsigned char* mask1 = nullptr;
  const unsigned char* mask2 = nullptr;
  if (pad_mask) {
    SA_HIP(hipMemcpyAsync(w_.mask, pad_mask, (size_t)Bi * T, hipMemcpyDeviceToDevice, st));
    SA_HIP(launch_repeat_rows_u8(pad_mask, w_.mask + (size_t)Bi * T, Bi, cand, T, st));
    mask1 = w_.mask;
    mask2 = w_.mask + (size_t)Bi * T;
  }
  // transformer(data_proj(codec features))                                             (judge.py:108-111)
  SA_TRY(enc_.forward(w_.xa, mask1, N1, T, st));
  const void* hid = enc_.out_act();  // [N1][S][D]; last_hidden_state = rows 1..T of each item
  // audio_features = cat_audio_proj(cat[hyp, inp])                                      (judge.py:112-115)
  const bool cat3 = (x3_ & SAMAUDIO_CLS_WO) != 0;
  const void* hid3 = nullptr;
  if (cat3) {   // the hidden states once in split form, into the encoder's D-wide scratch (free until the next forward)
    SA_TRY(x3_fits(enc_.x3_scratch(), enc_.x3_scratch_bytes(), (long)N1 * S, D, "judge_score: ", "the split operand does not fit the workspace plan"));
    SA_HIP(launch_split3(enc_.out_f32(), D, enc_.x3_scratch(), (long)N1 * S, D, st));
    hid3 = enc_.x3_scratch();
  }
  const X3Operand hid_op{hid3, nullptr, 0};   // (batched launches, rows 1..T of each item: offsets into the split copy)
  {
    GemmParams p = lin(hid, D, nullptr, T, Bn, D);  // mixture half, once per clip, with the bias
    p.nbatch = Bi; p.a_off = D; p.a_bstride = (long)S * D; p.bias = g_.cat_b;
    p.out_f32 = w_.inp_part; p.f32_ld = Bn; p.f32_bstride = (long)T * Bn;
    SA_TRY(enc_.linear(p, g_.cat_wi, SAMAUDIO_CLS_WO, hid_op, st));
    for (int c = 0; c < cand; ++c) {  // hypothesis half of candidate c of every clip + the clip's mixture half
      GemmParams q = lin(hid, D, nullptr, T, Bn, D);
      q.nbatch = Bi; q.a_off = ((long)(Bi + c) * S + 1) * D; q.a_bstride = (long)cand * S * D;
      q.res = w_.inp_part; q.res_ld = Bn; q.res_bstride = (long)T * Bn;
      q.out_act = w_.audio; q.act_ld = Bn; q.act_off = (long)c * T * Bn; q.act_bstride = (long)cand * T * Bn;
      SA_TRY(enc_.linear(q, g_.cat_wh, SAMAUDIO_CLS_WO, hid_op, st));
    }
  }
  // text branch: layer_norm(text_proj2(text_proj1(pooled)))                            (judge.py:98-100,116-120)
  SA_HIP(launch_to_act(text_pooled, 0, TH, 0, w_.tp_act, 0, bf16_, 1, Bp, TH, TH, 0, st));
  {
    GemmParams p = lin(w_.tp_act, TH, g_.tp1_w, Bp, D, TH);
    p.out_act = w_.t1; p.act_ld = D;
    SA_TRY(run_gemm(p, bf16_, "", st));
    p = lin(w_.t1, D, g_.tp2_w, Bp, Bn, D);
    p.bias = g_.tp2_b;
    p.out_f32 = w_.t2; p.f32_ld = Bn;
    SA_TRY(run_gemm(p, bf16_, "", st));
    SA_HIP(launch_layernorm_rows(w_.t2, Bn, g_.ln_w, g_.ln_b, nullptr, w_.tl, bf16_, Bp, Bn, 1e-5f, st));
    // text half of proj_audio_and_text, once per pair (the expanded text is constant over frames)
    p = lin(w_.tl, Bn, g_.pat_wt, Bp, Bn, Bn);
    p.bias = g_.pat_b;
    p.out_f32 = w_.tpart; p.f32_ld = Bn;
    SA_TRY(run_gemm(p, bf16_, "", st));
  }
  // audio_and_text = proj_audio_and_text(cat[audio_features, expanded_text])            (judge.py:121-123)
  {
    GemmParams p = lin(w_.audio, Bn, g_.pat_wa, T, Bn, Bn);
    p.nbatch = Bp; p.a_bstride = (long)T * Bn;
    p.res = w_.tpart; p.res_ld = 0; p.res_bstride = Bn;  // one row per pair, broadcast over its frames
    p.out_act = w_.at; p.act_ld = Bn; p.act_bstride = (long)T * Bn;
    SA_TRY(run_gemm(p, bf16_, "", st));
  }
  // finetune_transformer(finetune_data_proj(audio_and_text))                            (judge.py:124-126)
  SA_TRY(fin_.forward(w_.at, mask2, Bp, T, st));
  // head -> masked mean -> de-normalise                                                 (judge.py:127-132)
  SA_HIP(launch_judge_pool_head(fin_.out_f32(), fin_.seq_mask(), g_.head_w, g_.mean, g_.std_, scores, Bp, T, D2, st));
  return Status{};
}

Status Judge::encode(int which, const float* x, const unsigned char* pad_mask, int rows, int T, float* hidden,
                     hipStream_t st) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, "judge_encode: weights not finalized");
  if (which != 0 && which != 1) return fail(SAMAUDIO_ERR_ARG, "judge_encode: which must be 0 or 1");
  if (!x || !hidden || rows <= 0 || T <= 0) return fail(SAMAUDIO_ERR_ARG, "judge_encode: bad argument");
  PeavEncoder& e = which == 0 ? enc_ : fin_;
  Bump b(ws_, ws_bytes_);
  void* xa = b.take((size_t)rows * T * e.in_dim() * esz_);
  e.plan(b, rows, T, true);
  if (!ws_ || !b.fits())
    return fail(SAMAUDIO_ERR_WORKSPACE, "judge_encode: workspace too small (" + std::to_string(b.used()) + " bytes needed)");
  SA_HIP(launch_to_act(x, 0, e.in_dim(), 0, xa, 0, bf16_, 1, (long)rows * T, e.in_dim(), e.in_dim(), 0, st));
  SA_TRY(e.forward(xa, pad_mask, rows, T, st));
  SA_HIP(hipMemcpyAsync(hidden, e.out_f32(), (size_t)rows * (T + 1) * e.dim() * 4, hipMemcpyDeviceToDevice, st));
  return Status{};
}

// ---------------------------------------------------------------------------------------------------
// PE-A-Frame
// ---------------------------------------------------------------------------------------------------
FramePredictor::FramePredictor(const samaudio_frame_config& c)
    : cfg_(c), bf16_(c.precision == SAMAUDIO_BF16), esz_(bf16_ ? 2 : 4),
      at_dtype_(bf16_ ? SAMAUDIO_DT_BF16 : SAMAUDIO_DT_F32), enc_(with_in_dim(c.audio, c.codec_dim), bf16_, "a.") {}

Status FramePredictor::set_tensor(const char* name, const void* p, int dtype, int ndim, const int64_t* shape) {
  ready_ = false;
  return reg_.set(name, p, dtype, ndim, shape);
}

Status FramePredictor::set_option(int option, int value) {
  SA_TRY(check_x3_option(option, value, bf16_, "samaudio_frame_set_option"));
  x3_ = value;
  enc_.set_x3(value);
  ready_ = false;
  return Status{};
}

Status FramePredictor::finalize() {
  const int D = cfg_.audio.dim, E = cfg_.embed_dim;
  if (E <= 0 || E % 64 || cfg_.codec_dim % 64)
    return fail(SAMAUDIO_ERR_ARG, "frame: embed_dim / codec_dim must be positive multiples of 64");
  SA_TRY(enc_.finalize(reg_));
  const int AT = at_dtype_;
  NEEDF(reg_, g_.ah_ln_w, "ah.ln_w", D);   // audio_head: LayerNorm(eps 1e-6) + bias-free projection (hf:184-195)
  NEEDF(reg_, g_.ah_ln_b, "ah.ln_b", D);
  NEEDW(reg_, AT, g_.ah_w, "ah.w", E, D);
  NEEDF(reg_, g_.th_ln_w, "th.ln_w", E);   // text_audio_head
  NEEDF(reg_, g_.th_ln_b, "th.ln_b", E);
  NEEDW(reg_, AT, g_.th_w, "th.w", E, E);
  NEEDF(reg_, g_.scale, "logit_scale", 1);
  NEEDF(reg_, g_.bias, "logit_bias", 1);
  ready_ = true;
  return Status{};
}

void FramePredictor::plan(Bump& b, int rows, int T, bool assign) {
  const long D = cfg_.audio.dim, E = cfg_.embed_dim, CD = cfg_.codec_dim, S = T + 1, M = (long)rows * S;
  void* xa = b.take((size_t)rows * T * CD * esz_);
  void* a_ln = b.take((size_t)M * D * esz_);
  void* t_ln = b.take((size_t)rows * E * esz_);
  float* a_emb = (float*)b.take((size_t)M * E * 4);
  float* t_emb = (float*)b.take((size_t)rows * E * 4);
  if (assign) { w_.xa = xa; w_.a_ln = a_ln; w_.t_ln = t_ln; w_.a_emb = a_emb; w_.t_emb = t_emb; }
  enc_.plan(b, rows, T, assign);
}

size_t FramePredictor::workspace_bytes(int rows, int frames) {
  if (rows <= 0 || frames <= 0) return 0;
  Bump b;
  plan(b, rows, frames, false);
  return b.used() + 4096;
}

Status FramePredictor::set_workspace(void* p, size_t bytes) {
  if (!p || (reinterpret_cast<uintptr_t>(p) & 255)) return fail(SAMAUDIO_ERR_WORKSPACE, "workspace must be 256-byte aligned");
  ws_ = (char*)p;
  ws_bytes_ = bytes;
  return Status{};
}

Status FramePredictor::logits(const float* codec, const float* text_pooled, const unsigned char* pad_mask, int rows,
                              int T, float* out, hipStream_t st) {
  if (!ready_) return fail(SAMAUDIO_ERR_STATE, "frame_logits: weights not finalized");
  if (!codec || !text_pooled || !out || rows <= 0 || T <= 0) return fail(SAMAUDIO_ERR_ARG, "frame_logits: bad argument");
  Bump b(ws_, ws_bytes_);
  plan(b, rows, T, true);
  if (!ws_ || !b.fits())
    return fail(SAMAUDIO_ERR_WORKSPACE, "frame_logits: workspace too small (" + std::to_string(b.used()) + " bytes needed)");
  const int D = cfg_.audio.dim, E = cfg_.embed_dim, CD = cfg_.codec_dim, S = T + 1;
  const long M = (long)rows * S;
  SA_HIP(launch_to_act(codec, 0, CD, 0, w_.xa, 0, bf16_, 1, (long)rows * T, CD, CD, 0, st));
  SA_TRY(enc_.forward(w_.xa, pad_mask, rows, T, st));                                   // hf:640-680
  // audio_embeds = audio_head(last_hidden_state)   (class-token rows ride along and are skipped below)   hf:844-845
  SA_HIP(launch_layernorm_rows(enc_.out_f32(), D, g_.ah_ln_w, g_.ah_ln_b, nullptr, w_.a_ln, bf16_, M, D, 1e-6f, st));
  {
    GemmParams p = lin(w_.a_ln, D, g_.ah_w, M, E, D);
    p.out_f32 = w_.a_emb; p.f32_ld = E;
    SA_TRY(run_gemm(p, bf16_, "", st));
  }
  // text_audio_embeds = text_audio_head(text hidden state of token 0)                   hf:847-848
  SA_HIP(launch_layernorm_rows(text_pooled, E, g_.th_ln_w, g_.th_ln_b, nullptr, w_.t_ln, bf16_, rows, E, 1e-6f, st));
  {
    GemmParams p = lin(w_.t_ln, E, g_.th_w, rows, E, E);
    p.out_f32 = w_.t_emb; p.f32_ld = E;
    SA_TRY(run_gemm(p, bf16_, "", st));
  }
  // logits[b][t] = <audio_embeds[b][t], text_embeds[b]> * scale + bias                  hf:850-851, model.py:234-243
  SA_HIP(launch_frame_logits(w_.a_emb, (long)S * E, E, w_.t_emb, g_.scale, g_.bias, out, rows, T, E, st));
  return Status{};
}

}  // namespace sa
