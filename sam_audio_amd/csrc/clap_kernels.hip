// Kernels of the CLAP ranker towers that the GEMM / LayerNorm / attention kernels do not already cover (samaudio.h "CLAP ranker
// towers"; the definition is transformers' ClapModel, modeling_clap.py).  fp32 only.  HTSAT-tiny is a few
// GFLOP per clip beside an ODE solve of seconds, so these are plain latency-bound kernels: one wave per token or per window, no MFMA.
//   clap_patch_embed   normalised log-mel -> tokens: time interpolation, mel-to-image fold, patch convolution, LayerNorm; neither the
//                      interpolated nor the folded image is stored
//   swin_window_attn   shifted-window attention of one (clip, window, head): roll, partition, relative-position bias, region mask,
//                      softmax, PV, reverse and un-roll as index arithmetic on the q|k|v rows
//   swin_patch_merge   2 x 2 gather + LayerNorm(4 C) in front of the bias-free 4 C -> 2 C GEMM
//   clap_text_embed    RoBERTa's word + position + token-type embeddings (position ids from the running count of non-pad ids)
//   clap_score         <audio embedding, text embedding> per (clip, candidate)
#include "kernels.h"

namespace sa {

// torch's bicubic kernel (A = -0.75): the weights of the taps at floor(src) - 1 .. + 2 for the fraction t
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x3 = 2.f - t, u = 1.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

constexpr int kPatchMaxC = 1024;   // widest patch embedding (LDS row per wave)

// One wave per token (4 per workgroup).  Image (modeling_clap.py:761-795): row y = r F + f, column x  <-  frame r spec + x of the
// time axis interpolated to T' = spec * ratio frames (nn.functional.interpolate bicubic, align_corners=True: src = t' (frames - 1) /
// (T' - 1), taps clamped into the clip), mel bin f.  The source coordinate is evaluated in float64: one product per pixel.
__global__ __launch_bounds__(256) void clap_patch_embed_kernel(const float* __restrict__ feat, int n_tokens, int frames, int F, int spec,
                                                               int P, int S, int C, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                               const float* __restrict__ ln_b, float eps, float* __restrict__ tokens) {
  __shared__ float pix[4][64];
  __shared__ float val[4][kPatchMaxC];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long tok = (long)blockIdx.x * 4 + wv;
  const int G = spec / S, pad = (P - S) / 2, ratio = spec / F, Tp = spec * ratio;
  const bool active = tok < n_tokens;   // (no early return: the barriers below are workgroup-wide)
  if (active && lane < P * P) {
    const long b = tok / (G * G);
    const int g = (int)(tok - b * (G * G)), gy = g / G, gx = g - gy * G;
    const int y = gy * S - pad + lane / P, x = gx * S - pad + lane % P;
    float v = 0.f;
    if (y >= 0 && y < spec && x >= 0 && x < spec) {
      const int r = y / F, f = y - r * F, tp = r * spec + x;
      const float* src = feat + b * (long)frames * F + f;
      if (frames == Tp) {
        v = src[(long)tp * F];
      } else {
        const double pos = (double)tp * ((double)(frames - 1) / (double)(Tp - 1));
        const int i0 = (int)floor(pos);
        float cw[4];
        cubic_weights((float)(pos - (double)i0), cw);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          int i = i0 - 1 + k;
          i = i < 0 ? 0 : (i > frames - 1 ? frames - 1 : i);
          v = fmaf(cw[k], src[(long)i * F], v);
        }
      }
    }
    pix[wv][lane] = v;
  }
  __syncthreads();
  float sum = 0.f;
  if (active)
    for (int c = lane; c < C; c += 64) {
      float acc = bias[c];
      const float* wc = w + (long)c * P * P;
      for (int i = 0; i < P * P; ++i) acc = fmaf(wc[i], pix[wv][i], acc);
      val[wv][c] = acc;
      sum += acc;
    }
  if (!active) return;   // (a whole wave leaves together; nothing below is workgroup-wide)
  float* out = tokens + tok * C;
  if (!ln_w) {
    for (int c = lane; c < C; c += 64) out[c] = val[wv][c];
    return;
  }
  const float mean = wave_sum(sum) / C;
  float sq = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = val[wv][c] - mean;
    sq = fmaf(d, d, sq);
  }
  const float rstd = 1.f / sqrtf(wave_sum(sq) / C + eps);
  for (int c = lane; c < C; c += 64) out[c] = (val[wv][c] - mean) * rstd * ln_w[c] + ln_b[c];
}

hipError_t launch_clap_patch_embed(const float* feat, int n, int frames, int F, int spec, int P, int S, int C, const float* w,
                                   const float* bias, const float* ln_w, const float* ln_b, float eps, float* tokens, hipStream_t st) {
  if (n < 1 || S < 1 || P < S || P * P > 64 || C < 1 || C > kPatchMaxC || F < 1 || spec % F || spec % S || frames < 2 ||
      frames > spec * (spec / F))
    return hipErrorInvalidValue;
  const long n_tokens = (long)n * (spec / S) * (spec / S);
  if (n_tokens > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clap_patch_embed_kernel, dim3((unsigned)((n_tokens + 3) / 4)), dim3(256), 0, st, feat, (int)n_tokens, frames, F,
                     spec, P, S, C, w, bias, ln_w, ln_b, eps, tokens);
  return hipGetLastError();
}

// One wave per (clip, window, head); lane i is query token i of the window (ws^2 <= 64 tokens).  Token (iy, ix) of window (wy, wx)
// sits at (ys, xs) = (wy ws + iy, wx ws + ix) of the rolled map, i.e. at ((ys + shift) % H, (xs + shift) % W) of the token map
// (torch.roll by -shift, modeling_clap.py:583); the result goes back to that position (window_reverse and the roll by +shift).  The
// region of a token (modeling_clap.py:540-548) is taken on the rolled map: (ys >= H - ws) + (ys >= H - shift), the same along x;
// tokens of different regions get -100.
template <int HD>
__global__ __launch_bounds__(64) void swin_window_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                              float* __restrict__ out, int H, int W, int heads, int ws, int shift) {
  __shared__ float ks[64][HD + 1], vs[64][HD + 1];   // (+ 1: lane i fills row i, HD floats apart otherwise)
  __shared__ float sc[64][65];
  __shared__ int region[64];
  const int lane = threadIdx.x, wt = ws * ws, nwx = W / ws;
  const int head = blockIdx.x % heads, win = blockIdx.x / heads, wy = win / nwx, wx = win - wy * nwx;
  const long b = blockIdx.y, C = (long)heads * HD, ld = 3 * C;
  const int iy = lane / ws, ix = lane - iy * ws;
  float q[HD];
  long row = 0;
  if (lane < wt) {
    const int ys = wy * ws + iy, xs = wx * ws + ix;
    row = (b * H + (ys + shift) % H) * W + (xs + shift) % W;
    const float* src = qkv + row * ld + (long)head * HD;
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      q[d] = src[d];
      ks[lane][d] = src[C + d];
      vs[lane][d] = src[2 * C + d];
    }
    region[lane] = shift > 0 ? ((ys >= H - ws) + (ys >= H - shift)) * 3 + (xs >= W - ws) + (xs >= W - shift) : 0;
  }
  __syncthreads();
  if (lane >= wt) return;
  const float scale = 1.f / sqrtf((float)HD);
  const int span = 2 * ws - 1, mine = region[lane];
  float mx = -INFINITY;
  for (int j = 0; j < wt; ++j) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < HD; ++d) acc = fmaf(q[d], ks[j][d], acc);
    const int jy = j / ws, jx = j - jy * ws;
    float s = acc * scale + table[(long)((iy - jy + ws - 1) * span + (ix - jx + ws - 1)) * heads + head];
    if (region[j] != mine) s += -100.f;
    sc[lane][j] = s;
    mx = fmaxf(mx, s);
  }
  float den = 0.f;
  for (int j = 0; j < wt; ++j) {
    const float p = expf(sc[lane][j] - mx);
    sc[lane][j] = p;
    den += p;
  }
  const float inv = 1.f / den;
  float o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
  for (int j = 0; j < wt; ++j) {
    const float p = sc[lane][j] * inv;
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] = fmaf(p, vs[j][d], o[d]);
  }
  float* dst = out + row * C + (long)head * HD;
#pragma unroll
  for (int d = 0; d < HD; ++d) dst[d] = o[d];
}

hipError_t launch_swin_window_attn(const float* qkv, const float* table, float* out, int n, int H, int W, int heads, int hd, int ws,
                                   int shift, hipStream_t st) {
  if (n < 1 || n > 65535 || heads < 1 || ws < 1 || ws * ws > 64 || H % ws || W % ws || shift < 0 || shift >= ws || (hd != 24 && hd != 32))
    return hipErrorInvalidValue;
  const long blocks = (long)(H / ws) * (W / ws) * heads;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks, (unsigned)n);
  if (hd == 24) hipLaunchKernelGGL(swin_window_attn_kernel<24>, grid, dim3(64), 0, st, qkv, table, out, H, W, heads, ws, shift);
  else hipLaunchKernelGGL(swin_window_attn_kernel<32>, grid, dim3(64), 0, st, qkv, table, out, H, W, heads, ws, shift);
  return hipGetLastError();
}

// One wave per merged token (4 per workgroup): the four C-wide pieces in modeling_clap.py:709-711's order - (row, col) = (0, 0),
// (1, 0), (0, 1), (1, 1) - then LayerNorm over the 4 C values (two passes over L2-resident rows, then the write).
__global__ __launch_bounds__(256) void swin_patch_merge_kernel(const float* __restrict__ x, const float* __restrict__ ln_w,
                                                               const float* __restrict__ ln_b, float eps, float* __restrict__ out,
                                                               long n_out, int H, int W, int C) {
  const int lane = threadIdx.x & 63;
  const long tok = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_out) return;   // (no barrier in this kernel)
  const int H2 = H / 2, W2 = W / 2;
  const long b = tok / ((long)H2 * W2);
  const int g = (int)(tok - b * H2 * W2), oy = g / W2, ox = g - oy * W2;
  const float* piece[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) piece[k] = x + ((b * H + 2 * oy + (k & 1)) * W + 2 * ox + (k >> 1)) * (long)C;
  const int D = 4 * C;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int c = lane; c < C; c += 64) sum += piece[k][c];
  const float mean = wave_sum(sum) / D;
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int c = lane; c < C; c += 64) {
      const float d = piece[k][c] - mean;
      sq = fmaf(d, d, sq);
    }
  const float rstd = 1.f / sqrtf(wave_sum(sq) / D + eps);
  float* dst = out + tok * D;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int c = lane; c < C; c += 64) dst[k * C + c] = (piece[k][c] - mean) * rstd * ln_w[k * C + c] + ln_b[k * C + c];
}

hipError_t launch_swin_patch_merge(const float* x, const float* ln_w, const float* ln_b, float eps, float* out, int n, int H, int W,
                                   int C, hipStream_t st) {
  if (n < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || C < 1) return hipErrorInvalidValue;
  const long n_out = (long)n * (H / 2) * (W / 2);
  if ((n_out + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(swin_patch_merge_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, st, x, ln_w, ln_b, eps, out, n_out, H, W,
                     C);
  return hipGetLastError();
}

// One workgroup per row of ids.  position = pad + (ids != pad) * cumsum(ids != pad) (modeling_clap.py:1010): the cumulative count is
// one pass of a single thread over at most 1024 flags in LDS; then 256 threads copy-add the three embedding rows of every token.
__global__ __launch_bounds__(256) void clap_text_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ word,
                                                              const float* __restrict__ pos, const float* __restrict__ type,
                                                              float* __restrict__ out, int T, int D, int vocab, int pad) {
  __shared__ int position[1024];
  const long r = blockIdx.x;
  const long long* row = ids + r * T;
  for (int t = threadIdx.x; t < T; t += 256) position[t] = row[t] != pad ? 1 : 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    int count = 0;
    for (int t = 0; t < T; ++t) {
      count += position[t];
      position[t] = position[t] ? pad + count : pad;
    }
  }
  __syncthreads();
  for (long i = threadIdx.x; i < (long)T * D; i += 256) {
    const int t = (int)(i / D), d = (int)(i - (long)t * D);
    long long id = row[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);   // (the host refuses a token count the position table does not cover)
    out[(r * T + t) * D + d] = word[id * D + d] + type[d] + pos[(long)position[t] * D + d];
  }
}

hipError_t launch_clap_text_embed(const long long* ids, const float* word, const float* pos, const float* type, float* out, int rows,
                                  int T, int D, int vocab, int pad, hipStream_t st) {
  if (rows < 1 || T < 1 || T > 1024 || D < 1 || vocab < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clap_text_embed_kernel, dim3((unsigned)rows), dim3(256), 0, st, ids, word, pos, type, out, T, D, vocab, pad);
  return hipGetLastError();
}

__global__ __launch_bounds__(64) void clap_score_kernel(const float* __restrict__ audio, const float* __restrict__ text,
                                                        float* __restrict__ scores, int cand, int dim) {
  const long i = blockIdx.x;
  const float* a = audio + i * dim;
  const float* t = text + (i / cand) * dim;
  float s = 0.f;
  for (int d = threadIdx.x; d < dim; d += 64) s = fmaf(a[d], t[d], s);
  s = wave_sum(s);
  if (threadIdx.x == 0) scores[i] = s;
}

hipError_t launch_clap_score(const float* audio, const float* text, float* scores, int clips, int cand, int dim, hipStream_t st) {
  if (clips < 1 || cand < 1 || dim < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clap_score_kernel, dim3((unsigned)((long)clips * cand)), dim3(64), 0, st, audio, text, scores, cand, dim);
  return hipGetLastError();
}

}  // namespace sa
