// Streaming kernels of the PE-Core vision tower (reference
// sam_audio/model/vision_encoder.py:80-89 -> `pe.CLIP.encode_image`, architecture restated in oracle/vit_oracle.py).
// All of them are HBM-bound re-layouts around the GEMMs and the flash attention kernel (attention.hip):
//   patchify        frames [n,3,S,S] f32 -> im2col rows [n*G*G, Kp] (the k = stride = patch conv becomes one GEMM)
//   resize_frames   uint8 frames [n,3,H,W] -> resized, rounded, normalised: planar f32 or those im2col rows directly
//   resize_video    the same on frames picked by an index table from a video, with an object mask zeroing source pixels
//   rope2d_split    fused q|k|v rows -> Q, K [n,H,Sp,hd] with the 2-D rotary embedding, V^T [n,H,hd,Sp]
//   pool_attention  one learned query per head over all tokens (attention pooling head)
//   l2_normalize    rows of the projected features
#include "kernels.h"

#include "../../include/samaudio.h"   // SAMAUDIO_RESIZE_*

namespace sa {

// ------------------------------------------------------------------------------------------------
// im2col of a k = stride = P convolution: row (f, gy, gx), column k = c*P*P + py*P + px (the flattening of
// conv1.weight [W, 3, P, P]); columns >= 3*P*P are zero (K padded to the GEMM's slab).  grid (G*G, n), 256 threads.
// ------------------------------------------------------------------------------------------------
template <typename TA>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ frames, TA* __restrict__ out, int S,
                                                       int P, int G, int Kp) {
  const int patch = blockIdx.x, f = blockIdx.y;
  const int gy = patch / G, gx = patch - gy * G;
  const int kk = 3 * P * P;
  const float* src = frames + (long)f * 3 * S * S + (long)(gy * P) * S + gx * P;
  TA* dst = out + ((long)f * G * G + patch) * Kp;
  for (int k = threadIdx.x; k < Kp; k += 256) {
    float v = 0.f;
    if (k < kk) {
      const int c = k / (P * P), r = k - c * P * P;
      const int py = r / P, px = r - py * P;
      v = src[(long)c * S * S + (long)py * S + px];
    }
    Elem<TA>::store(dst + k, v);
  }
}

hipError_t launch_patchify(const float* frames, void* out, bool bf16, int n, int S, int P, int Kp, hipStream_t st) {
  const int G = S / P;
  dim3 grid(G * G, n), block(256);
  if (bf16) hipLaunchKernelGGL(patchify_kernel<bf16_t>, grid, block, 0, st, frames, (bf16_t*)out, S, P, G, Kp);
  else hipLaunchKernelGGL(patchify_kernel<float>, grid, block, 0, st, frames, (float*)out, S, P, G, Kp);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// resize_frames: uint8 frames [n,3,H,W] -> S x S, rounded to a level, normalised - what PerceptionEncoder.transform computes in torch:
// F.interpolate(x.float(), (S, S), mode, antialias=True, align_corners=False) -> round half to even -> clamp 0..255 ->
// (v / 255 - 0.5) / 0.5.  Output: planar f32 [n,3,S,S] (Kp == 0) or directly the im2col rows [n*G*G, Kp] of patchify_kernel
// (columns >= 3*P*P zero), so that neither a float copy of the source nor a planar intermediate ever reaches HBM.
//
// Per axis (in source pixels -> out = S), output index i:   scale = in / out, support = max(scale, 1) * r (r = 2 bicubic, 1 bilinear),
// inv = 1 / max(scale, 1), c = scale (i + 0.5), taps lo = max(0, int(c - support + 0.5)) .. hi = min(in, int(c + support + 0.5)),
// w_s = f((s - c + 0.5) inv) normalised to sum 1; f = triangle | cubic convolution with a = -0.5.  Nearest: the one tap
// min(floor(i * scale), in - 1).  lo / hi are formed in fp32 as torch forms them; the tap's distance to the centre is formed from the
// centre's integer part and fraction (fp64: in (2i + 1) / (2 out) is then exact), so the weights carry no error of a large fp32 c.
// The 2-D result is the horizontal pass followed by the vertical pass, both accumulated in fp32.
//
// One workgroup per (frame, channel, band of RZ_BAND output rows, tile of TX <= RZ_TX output columns).  It walks the source rows the
// band needs in chunks of RZ_HR, and inside a chunk the source columns the tile needs in chunks of RZ_CW: u8 rows are staged in LDS by
// aligned 16-byte loads (the row's misalignment is kept as a byte shift of the LDS row), the horizontal pass leaves fp32 rows in LDS,
// the vertical pass accumulates them into registers - any scale fits, a large one only loops longer.  Weights are formed in the kernel
// from the integer geometry: no tap table, no scratch.  Thread (xl, g) = (tid % TX, tid / TX): output column x0 + xl; source rows
// g, g + ng, ... of a chunk in the horizontal pass and output rows r0 + g, r0 + g + ng, ... in the vertical pass (ng = 256 / TX >= 2).
// grid (n * 3 * bands * tiles), 256 threads; static LDS 50 KB.
// ------------------------------------------------------------------------------------------------
constexpr int RZ_BAND = 14;              // output rows per workgroup
constexpr int RZ_TX = 128;               // most output columns per workgroup
constexpr int RZ_HR = 40;                // source rows per chunk
constexpr int RZ_CW = 768;               // source columns per chunk
constexpr int RZ_CWP = RZ_CW + 16;       // LDS row: the chunk behind a shift of up to 15 bytes, in whole 16-byte pieces
constexpr int RZ_NA = RZ_HR / 2;         // source rows of a chunk per thread (ng >= 2)
constexpr int RZ_NV = RZ_BAND / 2;       // output rows of the band per thread

struct ResizeTaps {
  int lo, hi;    // source pixels [lo, hi)
  int ci;        // centre: integer part ...
  float t, inv;  // ... and 0.5 - fraction; distance of source pixel s to the centre, in filter units = ((s - ci) + t) * inv
};

template <int MODE>
__device__ __forceinline__ ResizeTaps resize_taps(int in, int out, int i) {
  ResizeTaps p;
  const float scale = (float)in / (float)out;
  if (MODE == SAMAUDIO_RESIZE_NEAREST) {
    const int s = (int)floorf((float)i * scale);
    p.lo = s < in - 1 ? s : in - 1;
    p.hi = p.lo + 1; p.ci = p.lo; p.t = 0.f; p.inv = 1.f;
    return p;
  }
  const float support = (scale >= 1.f ? scale : 1.f) * (MODE == SAMAUDIO_RESIZE_BICUBIC ? 2.f : 1.f);
  const float c = scale * ((float)i + 0.5f);
  const int lo = (int)(c - support + 0.5f), hi = (int)(c + support + 0.5f);
  p.lo = lo > 0 ? lo : 0;
  p.hi = hi < in ? hi : in;
  p.inv = scale >= 1.f ? 1.f / scale : 1.f;
  const double cd = (double)in * (double)(2 * i + 1) / (2.0 * (double)out);
  p.ci = (int)cd;
  p.t = 0.5f - (float)(cd - (double)p.ci);
  return p;
}

template <int MODE>
__device__ __forceinline__ float resize_weight(const ResizeTaps& p, int s) {
  if (MODE == SAMAUDIO_RESIZE_NEAREST) return 1.f;
  const float x = fabsf(((float)(s - p.ci) + p.t) * p.inv);
  if (MODE == SAMAUDIO_RESIZE_BILINEAR) return x < 1.f ? 1.f - x : 0.f;
  constexpr float A = -0.5f;   // the antialiased bicubic filter's a (not the -0.75 of the plain one)
  if (x < 1.f) return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  if (x < 2.f) return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
  return 0.f;
}

// The video form (a ResizeVideo argument; samaudio_op_resize_video / samaudio_vit_encode_video): output frame f is computed from source
// frame pick[f] (null = f; clamped into [0, src_frames), so that no table can lead outside the tensors) of a video of src_frames frames,
// and a source pixel counts as 0 where its byte of `mask` [src_frames, mc, H, W] (mc = 1: one plane for the three channels | 3) is
// non-zero - the reference's `(v * m.eq(0))[idx]` without either copy.  The mask is applied while the aligned pieces are staged: a frame piece's 16
// bytes are source columns whose mask bytes start at the mask row's own (mis)alignment, so they are fetched as the one or two aligned
// 16-byte mask pieces that cover them, shifted into the frame's byte positions and turned into a byte-wise keep / zero - no second
// staging area in LDS, and everything behind the staging (taps, order, weights) is the code of the plain form: bit-identical to it on
// the materialised frames.  It is a compile-time property of the instantiation: the plain ones carry none of this.

// the aligned 16 bytes at mask + a (a % 16 == 0 in address terms) as two little-endian 64-bit words; bytes outside [0, mtotal) read 0
__device__ __forceinline__ void resize_mask_load(const unsigned char* __restrict__ mask, long mtotal, long a,
                                                 unsigned long long& w0, unsigned long long& w1) {
  if (a >= 0 && a + 16 <= mtotal) {
    const uint4 v = *(const uint4*)(mask + a);
    w0 = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    w1 = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    return;
  }
  w0 = w1 = 0ull;
  for (int e = 0; e < 16; ++e)
    if (a + e >= 0 && a + e < mtotal) {
      const unsigned long long m = (unsigned long long)mask[a + e] << (8 * (e & 7));
      if (e < 8) w0 |= m; else w1 |= m;
    }
}

// 0xFF in every byte of `m` that is non-zero, 0x00 elsewhere
__device__ __forceinline__ unsigned long long resize_mask_nonzero(unsigned long long m) {
  m |= m >> 4; m |= m >> 2; m |= m >> 1;   // bit 0 of a byte = the OR of its eight bits (what crosses a byte boundary lands above bit 0)
  return (m & 0x0101010101010101ull) * 0xFFull;
}

// the frame piece `v` with the bytes zeroed whose mask bytes mask[mb .. mb + 16) are non-zero (mb: any alignment, may lie partly outside)
__device__ __forceinline__ uint4 resize_mask_piece(uint4 v, const unsigned char* __restrict__ mask, long mtotal, long mb) {
  const int ms = (int)(((uintptr_t)mask + (uintptr_t)mb) & 15);
  unsigned long long l0, l1, l2 = 0ull, l3 = 0ull;
  resize_mask_load(mask, mtotal, mb - ms, l0, l1);
  if (ms) resize_mask_load(mask, mtotal, mb - ms + 16, l2, l3);
  if (ms >= 8) { l0 = l1; l1 = l2; l2 = l3; }
  const int bs = (ms & 7) * 8;
  const unsigned long long lo = bs ? (l0 >> bs) | (l1 << (64 - bs)) : l0, hi = bs ? (l1 >> bs) | (l2 << (64 - bs)) : l1;
  const unsigned long long klo = ~resize_mask_nonzero(lo), khi = ~resize_mask_nonzero(hi);
  v.x &= (unsigned)klo; v.y &= (unsigned)(klo >> 32);
  v.z &= (unsigned)khi; v.w &= (unsigned)(khi >> 32);
  return v;
}

struct ResizeVideo {
  const unsigned char* mask;   // [src_frames, mc, H, W] or null
  long mtotal;                 // its bytes
  const int* pick;             // [n] or null
  int src_frames, mc;
};

// VIDEO: nothing (the plain form: no further parameter, and none of the video form's code) or one ResizeVideo
template <int MODE, typename TA, typename... VIDEO>
__global__ __launch_bounds__(256) void resize_frames_kernel(const unsigned char* __restrict__ frames, long total,
                                                            TA* __restrict__ out, int H, int W, int S, int TX, int tiles,
                                                            int bands, int P, int Kp, VIDEO... video) {
  constexpr bool VID = sizeof...(VIDEO) != 0;
  static_assert(sizeof...(VIDEO) <= 1, "at most one ResizeVideo");
  ResizeVideo vd{nullptr, 0, nullptr, 0, 0};
  if constexpr (VID) vd = (video, ...);
  const unsigned char* __restrict__ mask = vd.mask;
  __shared__ __attribute__((aligned(16))) unsigned char src[RZ_HR * RZ_CWP];
  __shared__ float hrow[RZ_HR][RZ_TX];
  int wg = blockIdx.x;
  const int tile = wg % tiles; wg /= tiles;
  const int band = wg % bands; wg /= bands;
  const int c = wg % 3, f = wg / 3;
  const int r0 = band * RZ_BAND, r1 = r0 + RZ_BAND < S ? r0 + RZ_BAND : S;
  const int x0 = tile * TX, x1 = x0 + TX < S ? x0 + TX : S;
  if (x1 <= x0) return;   // (the whole workgroup)
  const int tid = threadIdx.x;
  const int ng = 256 / TX;
  const int xl = tid % TX, g = tid / TX;
  const bool active = g < ng && x0 + xl < x1;
  const int x = active ? x0 + xl : x0;
  const ResizeTaps hx = resize_taps<MODE>(W, S, x);
  // lo and hi do not decrease with the output index: the source window of the tile and of the band
  const int cl = resize_taps<MODE>(W, S, x0).lo, ch = resize_taps<MODE>(W, S, x1 - 1).hi;
  const int rl = resize_taps<MODE>(H, S, r0).lo, rh = resize_taps<MODE>(H, S, r1 - 1).hi;
  ResizeTaps vy[RZ_NV];
  float acc[RZ_NV], ws[RZ_NV];
#pragma unroll
  for (int a = 0; a < RZ_NV; ++a) {
    const int r = r0 + g + a * ng;
    vy[a] = resize_taps<MODE>(H, S, r < r1 ? r : r1 - 1);
    if (!active || r >= r1) vy[a].hi = vy[a].lo;   // no taps
    acc[a] = ws[a] = 0.f;
  }
  int fs = f;                                 // the source frame
  if (VID) {
    if (vd.pick) fs = vd.pick[f];
    fs = fs < 0 ? 0 : fs < vd.src_frames ? fs : vd.src_frames - 1;
  }
  const long plane = ((long)fs * 3 + c) * H;   // first source row of this (frame, channel)
  const long mplane = VID && mask ? ((long)fs * vd.mc + (vd.mc == 3 ? c : 0)) * H : 0;   // ... and of its mask plane
  constexpr int PCS = RZ_CWP / 16;            // 16-byte pieces per LDS row

  for (int j0 = rl; j0 < rh; j0 += RZ_HR) {
    const int nr = rh - j0 < RZ_HR ? rh - j0 : RZ_HR;
    float hacc[RZ_NA], hws = 0.f;
#pragma unroll
    for (int a = 0; a < RZ_NA; ++a) hacc[a] = 0.f;
    for (int q0 = cl; q0 < ch; q0 += RZ_CW) {
      const int nc = ch - q0 < RZ_CW ? ch - q0 : RZ_CW;
      // stage rows j0 .. j0 + nr, columns q0 .. q0 + nc: LDS row `row` holds them from byte (address of its first byte) & 15 on
      for (int idx = tid; idx < nr * PCS; idx += 256) {
        const int row = idx / PCS, pc = idx - row * PCS;
        const long o = (plane + j0 + row) * W + q0;
        const int sh = (int)((uintptr_t)(frames + o) & 15);
        if (pc * 16 < sh + nc) {
          const long b = o - sh + pc * 16;   // an aligned piece; it may begin before the tensor or end behind it
          uint4 v;
          if (b >= 0 && b + 16 <= total) {
            v = *(const uint4*)(frames + b);
          } else {
            unsigned w4[4] = {0u, 0u, 0u, 0u};
            for (int e = 0; e < 16; ++e)
              if (b + e >= 0 && b + e < total) w4[e >> 2] |= (unsigned)frames[b + e] << (8 * (e & 3));
            v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
          }
          if (VID && mask) v = resize_mask_piece(v, mask, vd.mtotal, (mplane + j0 + row) * W + q0 - sh + pc * 16);
          *(uint4*)(src + row * RZ_CWP + pc * 16) = v;
        }
      }
      __syncthreads();
      if (active) {
        int off[RZ_NA];   // LDS byte of (row, source column 0); rows past the chunk read row 0 and are dropped below
#pragma unroll
        for (int a = 0; a < RZ_NA; ++a) {
          const int row = g + a * ng < nr ? g + a * ng : 0;
          off[a] = row * RZ_CWP + (int)((uintptr_t)(frames + (plane + j0 + row) * W + q0) & 15) - q0;
        }
        const int s0 = hx.lo > q0 ? hx.lo : q0, s1 = hx.hi < q0 + nc ? hx.hi : q0 + nc;
        for (int s = s0; s < s1; ++s) {
          const float w = resize_weight<MODE>(hx, s);
          hws += w;
#pragma unroll
          for (int a = 0; a < RZ_NA; ++a) hacc[a] += w * (float)src[off[a] + s];
        }
      }
      __syncthreads();
    }
    if (active) {
      const float hn = hws != 0.f ? 1.f / hws : 0.f;
#pragma unroll
      for (int a = 0; a < RZ_NA; ++a)
        if (g + a * ng < nr) hrow[g + a * ng][xl] = hacc[a] * hn;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < RZ_NV; ++a) {
      const int s0 = vy[a].lo > j0 ? vy[a].lo : j0, s1 = vy[a].hi < j0 + nr ? vy[a].hi : j0 + nr;
      for (int s = s0; s < s1; ++s) {
        const float w = resize_weight<MODE>(vy[a], s);
        ws[a] += w;
        acc[a] += w * hrow[s - j0][xl];
      }
    }
    __syncthreads();
  }

  const int G = Kp ? S / P : 0, kk = 3 * P * P;
#pragma unroll
  for (int a = 0; a < RZ_NV; ++a) {
    const int r = r0 + g + a * ng;
    if (!active || r >= r1) continue;
    float v = ws[a] != 0.f ? acc[a] / ws[a] : 0.f;
    v = fminf(fmaxf(rintf(v), 0.f), 255.f);   // the level: round half to even, clamped (bicubic overshoot ends here)
    const float y = (v / 255.0f - 0.5f) / 0.5f;
    if (!Kp) {
      Elem<TA>::store(out + (((long)f * 3 + c) * S + r) * S + x, y);
      continue;
    }
    const int gy = r / P, py = r - gy * P, gx = x / P, px = x - gx * P;
    TA* dst = out + (((long)f * G + gy) * G + gx) * Kp;
    Elem<TA>::store(dst + c * P * P + py * P + px, y);
    if (c == 0 && py == 0 && px == 0)   // the patch's first pixel: its owner zeroes the K padding of the row
      for (int k = kk; k < Kp; ++k) Elem<TA>::store(dst + k, 0.f);
  }
}

template <int MODE>
static hipError_t launch_resize_frames_m(const unsigned char* frames, int n, int H, int W, int S, void* out, bool bf16, int P,
                                         int Kp, hipStream_t st) {
  const int tiles = (S + RZ_TX - 1) / RZ_TX, TX = (S + tiles - 1) / tiles, bands = (S + RZ_BAND - 1) / RZ_BAND;
  const long wgs = (long)n * 3 * bands * tiles, total = (long)n * 3 * H * W;
  if (wgs >= (1L << 24)) return hipErrorInvalidValue;
  dim3 grid((unsigned)wgs), block(256);
  if (bf16) hipLaunchKernelGGL((resize_frames_kernel<MODE, bf16_t>), grid, block, 0, st, frames, total, (bf16_t*)out, H, W, S, TX, tiles, bands, P, Kp);
  else hipLaunchKernelGGL((resize_frames_kernel<MODE, float>), grid, block, 0, st, frames, total, (float*)out, H, W, S, TX, tiles, bands, P, Kp);
  return hipGetLastError();
}

hipError_t launch_resize_frames(const unsigned char* frames, int n, int H, int W, int S, int mode, void* out, bool bf16, int P,
                                int Kp, hipStream_t st) {
  if (n <= 0 || H < 1 || W < 1 || S < 1 || (Kp && (P < 1 || S % P || Kp < 3 * P * P))) return hipErrorInvalidValue;
  if (mode == SAMAUDIO_RESIZE_NEAREST) return launch_resize_frames_m<SAMAUDIO_RESIZE_NEAREST>(frames, n, H, W, S, out, bf16, P, Kp, st);
  if (mode == SAMAUDIO_RESIZE_BILINEAR) return launch_resize_frames_m<SAMAUDIO_RESIZE_BILINEAR>(frames, n, H, W, S, out, bf16, P, Kp, st);
  if (mode == SAMAUDIO_RESIZE_BICUBIC) return launch_resize_frames_m<SAMAUDIO_RESIZE_BICUBIC>(frames, n, H, W, S, out, bf16, P, Kp, st);
  return hipErrorInvalidValue;
}

template <int MODE>
static hipError_t launch_resize_video_m(const unsigned char* frames, long src_frames, int H, int W, const unsigned char* mask, int mc,
                                        const int* pick, int n, int S, void* out, bool bf16, int P, int Kp, hipStream_t st) {
  const int tiles = (S + RZ_TX - 1) / RZ_TX, TX = (S + tiles - 1) / tiles, bands = (S + RZ_BAND - 1) / RZ_BAND;
  const long wgs = (long)n * 3 * bands * tiles, total = src_frames * 3 * H * W, mtotal = mask ? src_frames * mc * H * W : 0;
  if (wgs >= (1L << 24)) return hipErrorInvalidValue;
  dim3 grid((unsigned)wgs), block(256);
  const ResizeVideo vd{mask, mtotal, pick, (int)src_frames, mc};
  if (bf16) hipLaunchKernelGGL((resize_frames_kernel<MODE, bf16_t, ResizeVideo>), grid, block, 0, st, frames, total, (bf16_t*)out, H, W, S, TX, tiles, bands, P, Kp, vd);
  else hipLaunchKernelGGL((resize_frames_kernel<MODE, float, ResizeVideo>), grid, block, 0, st, frames, total, (float*)out, H, W, S, TX, tiles, bands, P, Kp, vd);
  return hipGetLastError();
}

hipError_t launch_resize_video(const unsigned char* frames, long src_frames, int H, int W, const unsigned char* mask, int mc,
                               const int* pick, int n, int S, int mode, void* out, bool bf16, int P, int Kp, hipStream_t st) {
  if (n <= 0 || src_frames < 1 || src_frames > 0x7fffffffL || H < 1 || W < 1 || S < 1 || (mask && mc != 1 && mc != 3) ||
      (!pick && n != src_frames) || (Kp && (P < 1 || S % P || Kp < 3 * P * P)))
    return hipErrorInvalidValue;
  if (mode == SAMAUDIO_RESIZE_NEAREST) return launch_resize_video_m<SAMAUDIO_RESIZE_NEAREST>(frames, src_frames, H, W, mask, mc, pick, n, S, out, bf16, P, Kp, st);
  if (mode == SAMAUDIO_RESIZE_BILINEAR) return launch_resize_video_m<SAMAUDIO_RESIZE_BILINEAR>(frames, src_frames, H, W, mask, mc, pick, n, S, out, bf16, P, Kp, st);
  if (mode == SAMAUDIO_RESIZE_BICUBIC) return launch_resize_video_m<SAMAUDIO_RESIZE_BICUBIC>(frames, src_frames, H, W, mask, mc, pick, n, S, out, bf16, P, Kp, st);
  return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------
// q|k|v rows [n*T, 3*H*HD] (bias already added by the GEMM) -> Q, K [n,H,Tp,HD] (rows t >= T zero) with the rotary
// embedding on adjacent pairs: (x0, x1) -> (x0 c - x1 s, x0 s + x1 c), c / s = rc / rs[t][pair] (tables [T][HD/2];
// null = no rotation); V -> V^T [n,H,HD,Tp].  grid (Tp/64, H, n), 256 threads.  Generic element type (fp32 parity path).
// ------------------------------------------------------------------------------------------------
template <typename TA, int HD>
__global__ __launch_bounds__(256) void rope2d_split_kernel(const TA* __restrict__ qkv, const float* __restrict__ rc,
                                                           const float* __restrict__ rs, TA* __restrict__ Q,
                                                           TA* __restrict__ K, TA* __restrict__ Vt, int T, int Tp, int H) {
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int D = H * HD;
  const long ld = 3L * D;
  const long bh = (long)b * H + h;
  constexpr int HP = HD / 2;
  for (int idx = threadIdx.x; idx < 64 * HP; idx += 256) {
    const int tt = idx / HP, pr = idx - tt * HP;
    const int t = t0 + tt;
    float q0 = 0.f, q1 = 0.f, k0 = 0.f, k1 = 0.f;
    if (t < T) {
      const TA* row = qkv + ((long)b * T + t) * ld + h * HD + 2 * pr;
      load2<TA>(row, q0, q1);
      load2<TA>(row + D, k0, k1);
      if (rc) {
        const float c = rc[(long)t * HP + pr], s = rs[(long)t * HP + pr];
        const float a0 = q0 * c - q1 * s, a1 = q0 * s + q1 * c;
        const float b0 = k0 * c - k1 * s, b1 = k0 * s + k1 * c;
        q0 = a0; q1 = a1; k0 = b0; k1 = b1;
      }
    }
    store2<TA>(Q + (bh * Tp + t) * HD + 2 * pr, q0, q1);
    store2<TA>(K + (bh * Tp + t) * HD + 2 * pr, k0, k1);
  }
  __shared__ float tile[64][HD + 1];
  for (int idx = threadIdx.x; idx < 64 * HD; idx += 256) {
    const int tt = idx / HD, d = idx - tt * HD;
    const int t = t0 + tt;
    tile[tt][d] = t < T ? Elem<TA>::load(qkv + ((long)b * T + t) * ld + 2L * D + h * HD + d) : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 64 * HD; idx += 256) {
    const int d = idx >> 6, tt = idx & 63;
    Elem<TA>::store(Vt + (bh * HD + d) * Tp + t0 + tt, tile[tt][d]);
  }
}

// bf16 fast path: HD/8 lanes x 16 bytes per head row, so every global access is a 16-byte load / store; the V tile is
// transposed through LDS as 16-bit words and leaves as 16-byte rows of V^T (same scheme as qkv_prep_bf16_kernel).
template <int HD>
__global__ __launch_bounds__(256) void rope2d_split_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ rc,
                                                                const float* __restrict__ rs, bf16_t* __restrict__ Q,
                                                                bf16_t* __restrict__ K, bf16_t* __restrict__ Vt, int T,
                                                                int Tp, int H) {
  constexpr int CH = HD / 8;         // 16-byte chunks per head row
  constexpr int RPI = 256 / CH;      // rows per iteration
  constexpr int VS = HD + 8;         // LDS row stride in shorts (spreads banks)
  __shared__ __attribute__((aligned(16))) unsigned short vt[64 * VS];
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int D = H * HD;
  const long ld = 3L * D;
  const int tid = threadIdx.x;
  const int sub = tid % CH, rgrp = tid / CH;
  const long bh = (long)b * H + h;
  auto unpack = [](const uint4& v, float (&x)[8]) {
    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[2 * e] = h16_lo(w4[e]);
      x[2 * e + 1] = h16_hi(w4[e]);
    }
  };
  auto pack = [](const float (&x)[8]) {
    // hardware conversion, as kernels.hip qkv_prep_bf16_kernel since round 4 (no SDWA rounding behind the packed-fp32 rotation)
    return make_uint4(pack_h16x2(x[0], x[1]), pack_h16x2(x[2], x[3]), pack_h16x2(x[4], x[5]), pack_h16x2(x[6], x[7]));
  };
#pragma unroll
  for (int it = 0; it < 64 / RPI; ++it) {
    const int tt = it * RPI + rgrp;
    const int t = t0 + tt;
    uint4 qo = make_uint4(0u, 0u, 0u, 0u), ko = qo, vv = qo;
    if (t < T) {
      const bf16_t* row = qkv + ((long)b * T + t) * ld + h * HD + sub * 8;
      qo = *(const uint4*)row;
      ko = *(const uint4*)(row + D);
      vv = *(const uint4*)(row + 2 * D);
      if (rc) {
        float q[8], k[8];
        unpack(qo, q);
        unpack(ko, k);
        const float4 c4 = *(const float4*)(rc + (long)t * (HD / 2) + sub * 4);
        const float4 s4 = *(const float4*)(rs + (long)t * (HD / 2) + sub * 4);
        const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a0 = q[2 * e], a1 = q[2 * e + 1];
          q[2 * e] = a0 * cc[e] - a1 * sn[e];
          q[2 * e + 1] = a0 * sn[e] + a1 * cc[e];
          const float b0 = k[2 * e], b1 = k[2 * e + 1];
          k[2 * e] = b0 * cc[e] - b1 * sn[e];
          k[2 * e + 1] = b0 * sn[e] + b1 * cc[e];
        }
        qo = pack(q);
        ko = pack(k);
      }
    }
    *(uint4*)(Q + (bh * Tp + t) * HD + sub * 8) = qo;
    *(uint4*)(K + (bh * Tp + t) * HD + sub * 8) = ko;
    *(uint4*)(vt + tt * VS + sub * 8) = vv;
  }
  __syncthreads();
  // V^T rows: item -> (d, 8 consecutive t); HD d x 8 chunks
#pragma unroll
  for (int it = 0; it < HD * 8 / 256; ++it) {
    const int item = it * 256 + tid;
    const int d = item >> 3, c = item & 7;
    unsigned short x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = vt[(c * 8 + e) * VS + d];
    const uint4 o = make_uint4((unsigned)x[0] | ((unsigned)x[1] << 16), (unsigned)x[2] | ((unsigned)x[3] << 16),
                               (unsigned)x[4] | ((unsigned)x[5] << 16), (unsigned)x[6] | ((unsigned)x[7] << 16));
    *(uint4*)(Vt + (bh * HD + d) * Tp + t0 + c * 8) = o;
  }
}

template <int HD>
static hipError_t launch_rope2d_split_t(const void* qkv, const float* rc, const float* rs, void* Q, void* K, void* Vt,
                                        bool bf16, int n, int T, int Tp, int H, hipStream_t st) {
  dim3 grid(Tp / 64, H, n), block(256);
  if (bf16)
    hipLaunchKernelGGL(rope2d_split_bf16_kernel<HD>, grid, block, 0, st, (const bf16_t*)qkv, rc, rs, (bf16_t*)Q, (bf16_t*)K,
                       (bf16_t*)Vt, T, Tp, H);
  else
    hipLaunchKernelGGL((rope2d_split_kernel<float, HD>), grid, block, 0, st, (const float*)qkv, rc, rs, (float*)Q,
                       (float*)K, (float*)Vt, T, Tp, H);
  return hipGetLastError();
}

hipError_t launch_rope2d_split(const void* qkv, const float* rc, const float* rs, void* Q, void* K, void* Vt, bool bf16,
                               int n, int T, int Tp, int H, int head_dim, hipStream_t st) {
  if (head_dim == 64) return launch_rope2d_split_t<64>(qkv, rc, rs, Q, K, Vt, bf16, n, T, Tp, H, st);
  if (head_dim == 128) return launch_rope2d_split_t<128>(qkv, rc, rs, Q, K, Vt, bf16, n, T, Tp, H, st);
  return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------------
// Attention pooling (AttentionPooling.forward -> nn.MultiheadAttention with ONE query): out[f, h*hd + :] =
// softmax_t(q_h . k[f, t, h] * hd^-0.5) . v[f, t, h];  q [H*hd] f32 is the same for every frame (probe through the
// q projection, precomputed at load); kv rows [n*T, 2*H*hd] = (k | v) from one GEMM.  One workgroup (4 waves) per
// (frame, head): a wave takes tokens w, w+4, ... with an online softmax, lane = 2 (hd = 128) or 1 (hd = 64) channels of
// the head; the four partial (m, l, o) states are merged through LDS.  grid (H, n), 256 threads.
// ------------------------------------------------------------------------------------------------
template <typename TA, int HD>
__global__ __launch_bounds__(256) void pool_attention_kernel(const float* __restrict__ q, const TA* __restrict__ kv,
                                                             TA* __restrict__ out, int T, int H) {
  constexpr int E = HD / 64;  // channels per lane
  const int h = blockIdx.x, f = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = H * HD;
  const float scale = HD == 128 ? 0.08838834764831845f : 0.125f;
  float qv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) qv[e] = q[h * HD + lane * E + e] * scale;
  float m = -INFINITY, l = 0.f, o[E];
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = 0.f;
  for (int t = wave; t < T; t += 4) {
    const TA* krow = kv + ((long)f * T + t) * (2L * D) + h * HD + lane * E;
    float kk[E], vv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { kk[e] = Elem<TA>::load(krow + e); vv[e] = Elem<TA>::load(krow + D + e); }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s += qv[e] * kk[e];
    s = wave_sum(s);
    const float m_new = fmaxf(m, s);
    const float a = expf(m - m_new), pv = expf(s - m_new);
    l = l * a + pv;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = o[e] * a + pv * vv[e];
    m = m_new;
  }
  __shared__ float sm[4], sl[4], so[4][HD];
  if (lane == 0) { sm[wave] = m; sl[wave] = l; }
#pragma unroll
  for (int e = 0; e < E; ++e) so[wave][lane * E + e] = o[e];
  __syncthreads();
  if (wave == 0) {
    float mm = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    float ll = 0.f, oo[E];
#pragma unroll
    for (int e = 0; e < E; ++e) oo[e] = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float a = sm[w] == -INFINITY ? 0.f : expf(sm[w] - mm);  // a wave with no token (T < 4) contributes nothing
      ll += sl[w] * a;
#pragma unroll
      for (int e = 0; e < E; ++e) oo[e] += so[w][lane * E + e] * a;
    }
    const float inv = 1.f / ll;
    if constexpr (E == 2) {   // one pair through store2 (hardware conversion for 16-bit outputs: common.h)
      store2<TA>(out + (long)f * D + h * HD + lane * E, oo[0] * inv, oo[1] * inv);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) Elem<TA>::store(out + (long)f * D + h * HD + lane * E + e, oo[e] * inv);
    }
  }
}

hipError_t launch_pool_attention(const float* q, const void* kv, void* out, bool bf16, int n, int T, int H, int head_dim,
                                 hipStream_t st) {
  dim3 grid(H, n), block(256);
  if (head_dim == 128) {
    if (bf16) hipLaunchKernelGGL((pool_attention_kernel<bf16_t, 128>), grid, block, 0, st, q, (const bf16_t*)kv, (bf16_t*)out, T, H);
    else hipLaunchKernelGGL((pool_attention_kernel<float, 128>), grid, block, 0, st, q, (const float*)kv, (float*)out, T, H);
  } else if (head_dim == 64) {
    if (bf16) hipLaunchKernelGGL((pool_attention_kernel<bf16_t, 64>), grid, block, 0, st, q, (const bf16_t*)kv, (bf16_t*)out, T, H);
    else hipLaunchKernelGGL((pool_attention_kernel<float, 64>), grid, block, 0, st, q, (const float*)kv, (float*)out, T, H);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// x[r, :] /= max(||x[r, :]||_2, 1e-12)   (F.normalize, `encode_image(normalize=True)`); one wave per row.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2_normalize_kernel(float* __restrict__ x, int rows, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float* xr = x + (long)row * D;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s += xr[i] * xr[i];
  const float inv = 1.f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
  for (int i = lane; i < D; i += 64) xr[i] *= inv;
}

hipError_t launch_l2_normalize(float* x, int rows, int D, hipStream_t st) {
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, rows, D);
  return hipGetLastError();
}

// mean over the T tokens of each frame: out[f, :] = AT(mean_t x[f, t, :])  (pool_type "avg"); grid (n), 256 threads
template <typename TO>
__global__ __launch_bounds__(256) void token_mean_kernel(const float* __restrict__ x, long x_ld, float* __restrict__ out_f32,
                                                         TO* __restrict__ out_act, int T, int D, int t_lo) {
  const int f = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += 256) {
    float acc = 0.f;
    for (int t = t_lo; t < T; ++t) acc += x[((long)f * T + t) * x_ld + d];
    acc /= (float)(T - t_lo);
    if (out_f32) out_f32[(long)f * D + d] = acc;
    if (out_act) Elem<TO>::store(out_act + (long)f * D + d, acc);
  }
}

hipError_t launch_token_mean(const float* x, long x_ld, float* out_f32, void* out_act, bool bf16, int n, int T, int D,
                             hipStream_t st) {
  if (bf16) hipLaunchKernelGGL(token_mean_kernel<bf16_t>, dim3(n), dim3(256), 0, st, x, x_ld, out_f32, (bf16_t*)out_act, T, D, 0);
  else hipLaunchKernelGGL(token_mean_kernel<float>, dim3(n), dim3(256), 0, st, x, x_ld, out_f32, (float*)out_act, T, D, 0);
  return hipGetLastError();
}

}  // namespace sa
