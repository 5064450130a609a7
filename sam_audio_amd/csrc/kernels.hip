// Bandwidth-bound kernels of the separate() path: norms, modulation, RoPE, layout changes.
// All of them are one-pass (or read-twice-from-L2) streaming kernels with 16-byte accesses where
// the layout allows; reductions are wave-shuffle based (64-lane wavefronts).
#include "kernels.h"

namespace sa {

static int g_debug_flags[64] = {0};
void set_debug_flag(int flag, int value) {
  if (flag >= 0 && flag < 64) g_debug_flags[flag] = value;
}
int debug_flag(int flag) { return flag >= 0 && flag < 64 ? g_debug_flags[flag] : 0; }

// ------------------------------------------------------------------------------------------------
// RMSNorm (+ adaLN modulate).  Reference transformer.py:36-47 (fp32 inside, eps in the rsqrt),
// :21-22 modulate = x*(1+scale)+shift, :360-372 / :507-518 where shift/scale = table + t-vector.
// One wave per row, 4 rows per workgroup.
// ------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void rmsnorm_mod_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ shift_tab,
                                                          const float* __restrict__ scale_tab,
                                                          const float* __restrict__ tvec, long tvec_ld, int shift_off,
                                                          int scale_off, TO* __restrict__ out, int M, int D,
                                                          int rows_per_b, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = (const float4*)(x + (long)row * D);
  const int n4 = D >> 2;
  float ss = 0.f;
  for (int i = lane; i < n4; i += 64) {
    float4 v = xr[i];
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = wave_sum(ss);
  const float inv = rsqrtf(ss / (float)D + eps);
  const float* trow = tvec ? tvec + (long)(row / rows_per_b) * tvec_ld : nullptr;
  TO* orow = out + (long)row * D;
  for (int i = lane; i < n4; i += 64) {
    float4 v = xr[i];
    float4 g = ((const float4*)w)[i];
    float o0 = v.x * inv * g.x, o1 = v.y * inv * g.y, o2 = v.z * inv * g.z, o3 = v.w * inv * g.w;
    if (trow) {
      float4 st = ((const float4*)shift_tab)[i], ct = ((const float4*)scale_tab)[i];
      float4 sv = *(const float4*)(trow + shift_off + 4 * i), cv = *(const float4*)(trow + scale_off + 4 * i);
      o0 = o0 * (1.f + (ct.x + cv.x)) + (st.x + sv.x);
      o1 = o1 * (1.f + (ct.y + cv.y)) + (st.y + sv.y);
      o2 = o2 * (1.f + (ct.z + cv.z)) + (st.z + sv.z);
      o3 = o3 * (1.f + (ct.w + cv.w)) + (st.w + sv.w);
    }
    store4<TO>(orow + 4 * i, o0, o1, o2, o3);
  }
}

// The shipped form for rows of D <= 256 * MAXV (launch_rmsnorm_mod): the row stays in registers between the statistics pass
// and the output pass (MAXV float4 per lane), so x is read from memory once instead of twice.  Same arithmetic order per
// lane as the kernel above, so results are bit-identical.
template <typename TO, int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_mod_reg_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ shift_tab,
                                                              const float* __restrict__ scale_tab,
                                                              const float* __restrict__ tvec, long tvec_ld, int shift_off,
                                                              int scale_off, TO* __restrict__ out, int M, int D,
                                                              int rows_per_b, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = (const float4*)(x + (long)row * D);
  const int n4 = D >> 2;
  float4 v[MAXV];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + 64 * k;
    v[k] = i < n4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    ss += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
  }
  ss = wave_sum(ss);
  const float inv = rsqrtf(ss / (float)D + eps);
  const float* trow = tvec ? tvec + (long)(row / rows_per_b) * tvec_ld : nullptr;
  TO* orow = out + (long)row * D;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + 64 * k;
    if (i >= n4) continue;
    float4 g = ((const float4*)w)[i];
    float o0 = v[k].x * inv * g.x, o1 = v[k].y * inv * g.y, o2 = v[k].z * inv * g.z, o3 = v[k].w * inv * g.w;
    if (trow) {
      float4 st = ((const float4*)shift_tab)[i], ct = ((const float4*)scale_tab)[i];
      float4 sv = *(const float4*)(trow + shift_off + 4 * i), cv = *(const float4*)(trow + scale_off + 4 * i);
      o0 = o0 * (1.f + (ct.x + cv.x)) + (st.x + sv.x);
      o1 = o1 * (1.f + (ct.y + cv.y)) + (st.y + sv.y);
      o2 = o2 * (1.f + (ct.z + cv.z)) + (st.z + sv.z);
      o3 = o3 * (1.f + (ct.w + cv.w)) + (st.w + sv.w);
    }
    store4<TO>(orow + 4 * i, o0, o1, o2, o3);
  }
}

// ------------------------------------------------------------------------------------------------
// RMSNorm + modulate with the per-evaluation operands pre-combined.  rmsnorm_mod above loads five column vectors per row
// (w, the layer's shift / scale tables, the evaluation's shift / scale vectors: 55 KB from L2 for 11 KB of row) and that
// costs 27 % of the kernel (34.2 vs 25.1 us without them at M = 8000, D = 2816, profiles/r2_call32/).  All five depend only
// on (layer, norm, time value), so one small launch per evaluation folds them into two vectors per norm,
//   g = w * (1 + (scale_tab + t_scale)),  s = shift_tab + t_shift,
// and the row kernel computes x * inv * g + s.  (Reassociates the reference's (x * inv * w) * (1 + scale) + shift:
// fp32 rounding differs in the last bit.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mod_tables_kernel(const ModTables t, const float* __restrict__ tvec, long tvec_ld,
                                                         float* __restrict__ gs, int D, int nt) {
  const int n = blockIdx.y, tt = blockIdx.z;   // norm index, time value
  const float* trow = tvec + (long)tt * tvec_ld;
  float* g = gs + (((long)n * nt + tt) * 2) * D;
  float* s = g + D;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < D; i += gridDim.x * 256) {
    const float sc = t.scale_tab[n][i] + trow[t.scale_off[n] + i];
    g[i] = t.w[n][i] * (1.f + sc);
    s[i] = t.shift_tab[n][i] + trow[t.shift_off[n] + i];
  }
}

hipError_t launch_mod_tables(const ModTables& t, int n_norms, const float* tvec, long tvec_ld, int nt, float* gs, int D,
                             hipStream_t st) {
  if (n_norms <= 0 || n_norms > kMaxModNorms) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mod_tables_kernel, dim3((D + 255) / 256, n_norms, nt), dim3(256), 0, st, t, tvec, tvec_ld, gs, D, nt);
  return hipGetLastError();
}

template <typename TO, int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_gs_reg_kernel(const float* __restrict__ x, const float* __restrict__ gs,
                                                             long gs_ld, TO* __restrict__ out, int M, int D, int rows_per_b,
                                                             float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = (const float4*)(x + (long)row * D);
  const int n4 = D >> 2;
  float4 v[MAXV];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + 64 * k;
    v[k] = i < n4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    ss += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
  }
  ss = wave_sum(ss);
  const float inv = rsqrtf(ss / (float)D + eps);
  const float4* g = (const float4*)(gs + (long)(row / rows_per_b) * gs_ld);
  const float4* s = g + n4;
  TO* orow = out + (long)row * D;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + 64 * k;
    if (i >= n4) continue;
    const float4 gg = g[i], sv = s[i];
    store4<TO>(orow + 4 * i, v[k].x * inv * gg.x + sv.x, v[k].y * inv * gg.y + sv.y, v[k].z * inv * gg.z + sv.z,
               v[k].w * inv * gg.w + sv.w);
  }
}

// the same row arithmetic with the result written as a compensated GEMM operand (split3_kernel's form): out [M, 3D] = [lo | hi | hi]
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_gs_split3_kernel(const float* __restrict__ x, const float* __restrict__ gs, long gs_ld,
                                                                bf16_t* __restrict__ out, int M, int D, int rows_per_b, float eps) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = (const float4*)(x + (long)row * D);
  const int n4 = D >> 2;
  float4 v[MAXV];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + 64 * k;
    v[k] = i < n4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    ss += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
  }
  ss = wave_sum(ss);
  const float inv = rsqrtf(ss / (float)D + eps);
  const float4* g = (const float4*)(gs + (long)(row / rows_per_b) * gs_ld);
  const float4* s = g + n4;
  bf16_t* orow = out + (long)row * 3 * D;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int i = lane + 64 * k;
    if (i >= n4) continue;
    const float4 gg = g[i], sv = s[i];
    const float o0 = v[k].x * inv * gg.x + sv.x, o1 = v[k].y * inv * gg.y + sv.y, o2 = v[k].z * inv * gg.z + sv.z,
                o3 = v[k].w * inv * gg.w + sv.w;
    const H16Split s0 = split_h16x2(o0, o1), s1 = split_h16x2(o2, o3);   // (common.h: the split of launch_split3)
    *(uint2*)(orow + 4 * i) = make_uint2(s0.lo, s1.lo);
    *(uint2*)(orow + D + 4 * i) = make_uint2(s0.hi, s1.hi);
    *(uint2*)(orow + 2 * D + 4 * i) = make_uint2(s0.hi, s1.hi);
  }
}
hipError_t launch_rmsnorm_gs_split3(const float* x, const float* gs, long gs_ld, void* out, int M, int D, int rows_per_b, float eps,
                                    hipStream_t st) {
  if (D > 256 * 12 || D % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rmsnorm_gs_split3_kernel<12>), dim3((M + 3) / 4), dim3(256), 0, st, x, gs, gs_ld, (bf16_t*)out, M, D, rows_per_b, eps);
  return hipGetLastError();
}

// gs = [g | s] of this norm for time value 0, gs_ld = floats between the time values (0: one time value for every row)
hipError_t launch_rmsnorm_gs(const float* x, const float* gs, long gs_ld, void* out, bool bf16, int M, int D, int rows_per_b,
                             float eps, hipStream_t st, bool out_alt) {
  if (D > 256 * 12 || D % 4) return hipErrorInvalidValue;
  dim3 grid((M + 3) / 4), block(256);
  if (bf16 && out_alt)   // mixed mode: the row feeds a GEMM on alt-format operands
    hipLaunchKernelGGL((rmsnorm_gs_reg_kernel<alt16_t, 12>), grid, block, 0, st, x, gs, gs_ld, (alt16_t*)out, M, D, rows_per_b, eps);
  else if (bf16)
    hipLaunchKernelGGL((rmsnorm_gs_reg_kernel<bf16_t, 12>), grid, block, 0, st, x, gs, gs_ld, (bf16_t*)out, M, D, rows_per_b, eps);
  else
    hipLaunchKernelGGL((rmsnorm_gs_reg_kernel<float, 12>), grid, block, 0, st, x, gs, gs_ld, (float*)out, M, D, rows_per_b, eps);
  return hipGetLastError();
}

hipError_t launch_rmsnorm_mod(const float* x, const float* w, const float* shift_tab, const float* scale_tab,
                              const float* tvec, long tvec_ld, int shift_off, int scale_off, void* out, bool bf16,
                              int M, int D, int rows_per_b, float eps, hipStream_t st) {
  dim3 grid((M + 3) / 4), block(256);
  // the row stays in registers between the statistics pass and the output pass (one read of x; bit-identical to the
  // two-pass kernel): 34.3 vs 37.6 us at M = 8000, D = 2816 on MI355X (profiles/r2_op_bench_first.log); wider rows take
  // the two-pass kernel below
  if (D <= 256 * 12) {
    if (bf16)
      hipLaunchKernelGGL((rmsnorm_mod_reg_kernel<bf16_t, 12>), grid, block, 0, st, x, w, shift_tab, scale_tab, tvec, tvec_ld,
                         shift_off, scale_off, (bf16_t*)out, M, D, rows_per_b, eps);
    else
      hipLaunchKernelGGL((rmsnorm_mod_reg_kernel<float, 12>), grid, block, 0, st, x, w, shift_tab, scale_tab, tvec, tvec_ld,
                         shift_off, scale_off, (float*)out, M, D, rows_per_b, eps);
    return hipGetLastError();
  }
  if (bf16)
    hipLaunchKernelGGL(rmsnorm_mod_kernel<bf16_t>, grid, block, 0, st, x, w, shift_tab, scale_tab, tvec, tvec_ld,
                       shift_off, scale_off, (bf16_t*)out, M, D, rows_per_b, eps);
  else
    hipLaunchKernelGGL(rmsnorm_mod_kernel<float>, grid, block, 0, st, x, w, shift_tab, scale_tab, tvec, tvec_ld,
                       shift_off, scale_off, (float*)out, M, D, rows_per_b, eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// acc += tanh(gate) * LayerNorm(x)   (reference align.py:41-50; eps = torch default 1e-5)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layernorm_accum_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, const float* __restrict__ gate,
                                                              float* __restrict__ acc, int M, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const float4* xr = (const float4*)(x + (long)row * D);
  const int n4 = D >> 2;
  float s = 0.f;
  for (int i = lane; i < n4; i += 64) {
    float4 v = xr[i];
    s += v.x + v.y + v.z + v.w;
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int i = lane; i < n4; i += 64) {
    float4 v = xr[i];
    float a = v.x - mean, c = v.y - mean, d = v.z - mean, e = v.w - mean;
    q += a * a + c * c + d * d + e * e;
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
  const float g = tanhf(gate[0]);
  float4* ar = (float4*)(acc + (long)row * D);
  for (int i = lane; i < n4; i += 64) {
    float4 v = xr[i], ww = ((const float4*)w)[i], bb = ((const float4*)b)[i], a = ar[i];
    a.x += g * ((v.x - mean) * rstd * ww.x + bb.x);
    a.y += g * ((v.y - mean) * rstd * ww.y + bb.y);
    a.z += g * ((v.z - mean) * rstd * ww.z + bb.z);
    a.w += g * ((v.w - mean) * rstd * ww.w + bb.w);
    ar[i] = a;
  }
}

hipError_t launch_layernorm_accum(const float* x, const float* w, const float* b, const float* gate, float* acc,
                                  int M, int D, float eps, hipStream_t st) {
  hipLaunchKernelGGL(layernorm_accum_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, w, b, gate, acc, M, D, eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// GroupNorm(num_groups=1) + SiLU, channels-last (reference patcher.py:83-101 with num_groups=1,
// :155-159; statistics over C x T per sample, padded frames included - quirk Q5).
// Pass 1: GN_CHUNKS partial (sum, sumsq) per sample in fp64, fixed order (deterministic);
// pass 2: every workgroup folds the partials (same order everywhere) and streams its rows.
// ------------------------------------------------------------------------------------------------
constexpr int GN_CHUNKS = 64;

__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, double* __restrict__ partials,
                                                         long per_sample) {
  const int b = blockIdx.y, c = blockIdx.x;
  const long n4 = per_sample >> 2;
  const long per_chunk = (n4 + GN_CHUNKS - 1) / GN_CHUNKS;
  const long lo = c * per_chunk, hi = (lo + per_chunk < n4) ? lo + per_chunk : n4;
  const float4* xs = (const float4*)(x + (long)b * per_sample);
  double s = 0.0, q = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    float4 v = xs[i];
    s += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
    q += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  __shared__ double sh[2][256];
  sh[0][threadIdx.x] = s;
  sh[1][threadIdx.x] = q;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partials[((long)b * GN_CHUNKS + c) * 2 + 0] = sh[0][0];
    partials[((long)b * GN_CHUNKS + c) * 2 + 1] = sh[1][0];
  }
}

template <typename TO>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       const double* __restrict__ partials, TO* __restrict__ out,
                                                       int T, int C, int halo, float eps) {
  const int b = blockIdx.y;
  double s = 0.0, q = 0.0;
  for (int c = 0; c < GN_CHUNKS; ++c) {
    s += partials[((long)b * GN_CHUNKS + c) * 2 + 0];
    q += partials[((long)b * GN_CHUNKS + c) * 2 + 1];
  }
  const double n = (double)T * (double)C;
  const double mean_d = s / n;
  double var_d = q / n - mean_d * mean_d;
  if (var_d < 0.0) var_d = 0.0;
  const float mean = (float)mean_d, rstd = (float)(1.0 / sqrt(var_d + (double)eps));
  const int n4 = C >> 2;
  const long total4 = (long)T * n4;
  const float4* xs = (const float4*)(x + (long)b * T * C);
  TO* ob = out + ((long)b * (T + 2 * halo) + halo) * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const int c4 = (int)(i % n4);
    float4 v = xs[i], ww = ((const float4*)w)[c4], bb = ((const float4*)bias)[c4];
    store4<TO>(ob + 4 * i, silu_f((v.x - mean) * rstd * ww.x + bb.x), silu_f((v.y - mean) * rstd * ww.y + bb.y),
               silu_f((v.z - mean) * rstd * ww.z + bb.z), silu_f((v.w - mean) * rstd * ww.w + bb.w));
  }
}

hipError_t launch_groupnorm_silu(const float* x, const float* w, const float* b, double* partials, void* out,
                                 bool bf16, int B, int T, int C, int halo, float eps, hipStream_t st) {
  hipLaunchKernelGGL(gn_partial_kernel, dim3(GN_CHUNKS, B), dim3(256), 0, st, x, partials, (long)T * C);
  long total4 = (long)T * (C / 4);
  int gx = (int)((total4 + 255) / 256);
  if (gx > 512) gx = 512;
  if (bf16)
    hipLaunchKernelGGL(gn_apply_kernel<bf16_t>, dim3(gx, B), dim3(256), 0, st, x, w, b, partials, (bf16_t*)out, T, C,
                       halo, eps);
  else
    hipLaunchKernelGGL(gn_apply_kernel<float>, dim3(gx, B), dim3(256), 0, st, x, w, b, partials, (float*)out, T, C,
                       halo, eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// QKV post-processing (reference transformer.py:139-151 + rope.py:145-155):
//   q,k: per-head RMSNorm over 128 (weight shared by all heads) then RoPE on adjacent pairs (2i,2i+1),
//        written as [B,H,Tp,128] (rows t >= T are zero);
//   v  : transposed to [B,H,128,Tp] so that P@V is a K-contiguous ("NT") MFMA contraction.
// The QKV GEMM already produces head-major columns (weights permuted at load, quirk Q1).
// grid (Tp/64, H, B), 256 threads.
// ------------------------------------------------------------------------------------------------
// HD = head_dim (128: every lane of the wave holds one adjacent pair of the head row; 64: lanes 32 .. 63 sit out - the general
// form for DiT configurations whose dim / n_heads is 64, reference transformer.py:100-119; the 16-byte fast path below is 128 only)
template <typename TA, int HD>
__global__ __launch_bounds__(256) void qkv_prep_kernel(const TA* __restrict__ qkv, const float* __restrict__ qw,
                                                       const float* __restrict__ kw, const float* __restrict__ rc,
                                                       const float* __restrict__ rs, TA* __restrict__ Q,
                                                       TA* __restrict__ K, TA* __restrict__ Vt, int T, int Tp, int H,
                                                       float eps) {
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int D = H * HD;
  const long ld = 3L * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool on = lane < HD / 2;
  const long bh = (long)b * H + h;
  const float w0q = on ? qw[2 * lane] : 0.f, w1q = on ? qw[2 * lane + 1] : 0.f;
  const float w0k = on ? kw[2 * lane] : 0.f, w1k = on ? kw[2 * lane + 1] : 0.f;
  for (int i = 0; i < 16; ++i) {
    const int t = t0 + wave * 16 + i;
    float q0 = 0.f, q1 = 0.f, k0 = 0.f, k1 = 0.f;
    if (t < T) {
      if (on) {
        const TA* row = qkv + ((long)b * T + t) * ld + h * HD + 2 * lane;
        load2<TA>(row, q0, q1);
        load2<TA>(row + D, k0, k1);
      }
      const float iq = rsqrtf(wave_sum(q0 * q0 + q1 * q1) / (float)HD + eps);
      const float ik = rsqrtf(wave_sum(k0 * k0 + k1 * k1) / (float)HD + eps);
      q0 *= iq * w0q; q1 *= iq * w1q; k0 *= ik * w0k; k1 *= ik * w1k;
      const float c = on ? rc[(long)t * (HD / 2) + lane] : 1.f, s = on ? rs[(long)t * (HD / 2) + lane] : 0.f;
      const float a0 = q0 * c - q1 * s, a1 = q0 * s + q1 * c;
      const float b0 = k0 * c - k1 * s, b1 = k0 * s + k1 * c;
      q0 = a0; q1 = a1; k0 = b0; k1 = b1;
    }
    if (on) {
      store2<TA>(Q + (bh * Tp + t) * HD + 2 * lane, q0, q1);
      store2<TA>(K + (bh * Tp + t) * HD + 2 * lane, k0, k1);
    }
  }
  __shared__ float tile[64][HD + 1];
  for (int idx = threadIdx.x; idx < 64 * HD; idx += 256) {
    const int tt = idx / HD, d = idx % HD;
    const int t = t0 + tt;
    tile[tt][d] = t < T ? Elem<TA>::load(qkv + ((long)b * T + t) * ld + 2L * D + h * HD + d) : 0.f;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 64 * HD; idx += 256) {
    const int d = idx >> 6, tt = idx & 63;
    Elem<TA>::store(Vt + (bh * HD + d) * Tp + t0 + tt, tile[tt][d]);
  }
}

// bf16 fast path: 16 lanes x 16 bytes per 128-wide head row (4 rows per wave-instruction), so every global access
// is a 16-byte load / store; the V tile is transposed through LDS as 16-bit words and leaves as 16-byte rows of V^T.
// SWROUND = false (shipped): the 16-bit rounding of Q / K is the hardware conversion (pack_h16x2: v_cvt_pk_bf16_f32 / v_cvt_f16_f32).
// SWROUND = true (DBG_QKV_PREP_SWROUND = 1) is the form this kernel had until round 4, kept as the reproducer of what it did: written out
// (f2bf: integer add of 0x7fff + lsb), hipcc turns the bf16 rounding into SDWA word-select instructions (v_and_b32_sdwa ...
// src0_sel:WORD_1) directly behind the packed-fp32 rotation (v_pk_fma_f32) that produces their operand - and when another kernel's waves
// share the SIMD, the high half of one dword of Q (element 5 of a lane's 8) comes out wrong in ~0.5 % of the launches: 208 of 40 000
// with a second stream busy, 0 of 40 000 alone, 0 of 40 000 with the hardware conversion, 0 of 40 000 with two idle cycles between
// rotation and rounding, never in K or V^T, never in the fp16 build (whose f2bf is the hardware conversion anyway) -
// tools/stress_qkv_prep.py, profiles/r4_call20/, r4_call21/.  This was the run-to-run difference of SAMAudio(streams=2) that rounds 3
// and 4 chased: the per-stage checksum trace put all 26 sightings at this kernel's Q output.  Same bits as f2bf
// for every finite value (the kernel's tests, and 40 000 launches against torch fp32 on the device).
template <bool SWROUND>
__global__ __launch_bounds__(256) void qkv_prep_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ qw,
                                                            const float* __restrict__ kw, const float* __restrict__ rc,
                                                            const float* __restrict__ rs, bf16_t* __restrict__ Q,
                                                            bf16_t* __restrict__ K, bf16_t* __restrict__ Vt, int T,
                                                            int Tp, int H, float eps) {
  __shared__ __attribute__((aligned(16))) unsigned short vt[64 * 136];  // [t][d], row stride 136 (272 B) spreads banks
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int D = H * 128;
  const long ld = 3L * D;
  const int tid = threadIdx.x;
  const int sub = tid & 15;   // 8-element chunk of the head row
  const int rgrp = tid >> 4;  // 16 row groups
  const long bh = (long)b * H + h;
  float wq[8], wk[8];
  {
    const float4 a = *(const float4*)(qw + sub * 8), c = *(const float4*)(qw + sub * 8 + 4);
    const float4 e = *(const float4*)(kw + sub * 8), f = *(const float4*)(kw + sub * 8 + 4);
    wq[0] = a.x; wq[1] = a.y; wq[2] = a.z; wq[3] = a.w; wq[4] = c.x; wq[5] = c.y; wq[6] = c.z; wq[7] = c.w;
    wk[0] = e.x; wk[1] = e.y; wk[2] = e.z; wk[3] = e.w; wk[4] = f.x; wk[5] = f.y; wk[6] = f.z; wk[7] = f.w;
  }
  auto unpack = [](const uint4& v, float (&x)[8]) {
    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[2 * e] = h16_lo(w4[e]);
      x[2 * e + 1] = h16_hi(w4[e]);
    }
  };
  auto pack = [](const float (&x)[8]) {
    if constexpr (!SWROUND)
      return make_uint4(pack_h16x2(x[0], x[1]), pack_h16x2(x[2], x[3]), pack_h16x2(x[4], x[5]), pack_h16x2(x[6], x[7]));
    else
      return make_uint4((unsigned)f2bf(x[0]) | ((unsigned)f2bf(x[1]) << 16), (unsigned)f2bf(x[2]) | ((unsigned)f2bf(x[3]) << 16),
                        (unsigned)f2bf(x[4]) | ((unsigned)f2bf(x[5]) << 16), (unsigned)f2bf(x[6]) | ((unsigned)f2bf(x[7]) << 16));
  };
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int tt = it * 16 + rgrp;
    const int t = t0 + tt;
    uint4 qo = make_uint4(0u, 0u, 0u, 0u), ko = qo, vv = qo;
    if (t < T) {  // uniform over each 16-lane row group
      const bf16_t* row = qkv + ((long)b * T + t) * ld + h * 128 + sub * 8;
      const uint4 qi = *(const uint4*)row, ki = *(const uint4*)(row + D);
      vv = *(const uint4*)(row + 2 * D);
      float q[8], k[8];
      unpack(qi, q);
      unpack(ki, k);
      float sq = 0.f, sk = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { sq += q[e] * q[e]; sk += k[e] * k[e]; }
      sq = row16_sum(sq);
      sk = row16_sum(sk);
      const float iq = rsqrtf(sq / 128.f + eps), ik = rsqrtf(sk / 128.f + eps);
      const float4 c4 = *(const float4*)(rc + (long)t * 64 + sub * 4), s4 = *(const float4*)(rs + (long)t * 64 + sub * 4);
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a0 = q[2 * e] * iq * wq[2 * e], a1 = q[2 * e + 1] * iq * wq[2 * e + 1];
        q[2 * e] = a0 * cc[e] - a1 * sn[e];
        q[2 * e + 1] = a0 * sn[e] + a1 * cc[e];
        const float b0 = k[2 * e] * ik * wk[2 * e], b1 = k[2 * e + 1] * ik * wk[2 * e + 1];
        k[2 * e] = b0 * cc[e] - b1 * sn[e];
        k[2 * e + 1] = b0 * sn[e] + b1 * cc[e];
      }
      qo = pack(q);
      ko = pack(k);
    }
    *(uint4*)(Q + (bh * Tp + t) * 128 + sub * 8) = qo;
    *(uint4*)(K + (bh * Tp + t) * 128 + sub * 8) = ko;
    *(uint4*)(vt + tt * 136 + sub * 8) = vv;
  }
  __syncthreads();
  // V^T rows: thread -> (d, 8 consecutive t); 128 d x 8 chunks = 1024 items, 4 per thread
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int item = it * 256 + tid;
    const int d = item >> 3, c = item & 7;
    unsigned short x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = vt[(c * 8 + e) * 136 + d];
    const uint4 o = make_uint4((unsigned)x[0] | ((unsigned)x[1] << 16), (unsigned)x[2] | ((unsigned)x[3] << 16),
                               (unsigned)x[4] | ((unsigned)x[5] << 16), (unsigned)x[6] | ((unsigned)x[7] << 16));
    *(uint4*)(Vt + (bh * 128 + d) * Tp + t0 + c * 8) = o;
  }
}

// fp32 form of the fast path above (x3 contexts: fp32 qkv rows in, fp32 Q / K / V^T out for the compensated self-attention): 16
// lanes x 32 bytes per 128-wide head row, row statistics by 16-lane DPP reductions, V transposed through LDS.  The general fp32
// kernel above - one wave per row, two 64-lane reductions after one another - stays the exact-fp32 parity mode's (its summation
// order is what the fp32 golden tests were recorded with); this one runs 56 us per launch at M = 4 000 where the generic one took 90 (profiles/r6_final2/ -> r6_final3/).
__global__ __launch_bounds__(256) void qkv_prep_f32x_kernel(const float* __restrict__ qkv, const float* __restrict__ qw,
                                                            const float* __restrict__ kw, const float* __restrict__ rc,
                                                            const float* __restrict__ rs, float* __restrict__ Q, float* __restrict__ K,
                                                            float* __restrict__ Vt, int T, int Tp, int H, float eps) {
  __shared__ __attribute__((aligned(16))) float vt[64 * 132];  // [t][d], row stride 132 floats
  const int t0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int D = H * 128;
  const long ld = 3L * D;
  const int tid = threadIdx.x;
  const int sub = tid & 15;   // 8-element chunk of the head row
  const int rgrp = tid >> 4;  // 16 row groups
  const long bh = (long)b * H + h;
  float wq[8], wk[8];
  {
    const float4 a = *(const float4*)(qw + sub * 8), c = *(const float4*)(qw + sub * 8 + 4);
    const float4 e = *(const float4*)(kw + sub * 8), f = *(const float4*)(kw + sub * 8 + 4);
    wq[0] = a.x; wq[1] = a.y; wq[2] = a.z; wq[3] = a.w; wq[4] = c.x; wq[5] = c.y; wq[6] = c.z; wq[7] = c.w;
    wk[0] = e.x; wk[1] = e.y; wk[2] = e.z; wk[3] = e.w; wk[4] = f.x; wk[5] = f.y; wk[6] = f.z; wk[7] = f.w;
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int tt = it * 16 + rgrp;
    const int t = t0 + tt;
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, k[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (t < T) {  // uniform over each 16-lane row group
      const float* row = qkv + ((long)b * T + t) * ld + h * 128 + sub * 8;
      const float4 q0 = *(const float4*)row, q1 = *(const float4*)(row + 4), k0 = *(const float4*)(row + D), k1 = *(const float4*)(row + D + 4);
      v0 = *(const float4*)(row + 2 * D);
      v1 = *(const float4*)(row + 2 * D + 4);
      q[0] = q0.x; q[1] = q0.y; q[2] = q0.z; q[3] = q0.w; q[4] = q1.x; q[5] = q1.y; q[6] = q1.z; q[7] = q1.w;
      k[0] = k0.x; k[1] = k0.y; k[2] = k0.z; k[3] = k0.w; k[4] = k1.x; k[5] = k1.y; k[6] = k1.z; k[7] = k1.w;
      float sq = 0.f, sk = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) { sq += q[e] * q[e]; sk += k[e] * k[e]; }
      sq = row16_sum(sq);
      sk = row16_sum(sk);
      const float iq = rsqrtf(sq / 128.f + eps), ik = rsqrtf(sk / 128.f + eps);
      const float4 c4 = *(const float4*)(rc + (long)t * 64 + sub * 4), s4 = *(const float4*)(rs + (long)t * 64 + sub * 4);
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, sn[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a0 = q[2 * e] * iq * wq[2 * e], a1 = q[2 * e + 1] * iq * wq[2 * e + 1];
        q[2 * e] = a0 * cc[e] - a1 * sn[e];
        q[2 * e + 1] = a0 * sn[e] + a1 * cc[e];
        const float b0 = k[2 * e] * ik * wk[2 * e], b1 = k[2 * e + 1] * ik * wk[2 * e + 1];
        k[2 * e] = b0 * cc[e] - b1 * sn[e];
        k[2 * e + 1] = b0 * sn[e] + b1 * cc[e];
      }
    }
    float* qd = Q + (bh * Tp + t) * 128 + sub * 8;
    float* kd = K + (bh * Tp + t) * 128 + sub * 8;
    *(float4*)qd = make_float4(q[0], q[1], q[2], q[3]);
    *(float4*)(qd + 4) = make_float4(q[4], q[5], q[6], q[7]);
    *(float4*)kd = make_float4(k[0], k[1], k[2], k[3]);
    *(float4*)(kd + 4) = make_float4(k[4], k[5], k[6], k[7]);
    *(float4*)(vt + tt * 132 + sub * 8) = v0;
    *(float4*)(vt + tt * 132 + sub * 8 + 4) = v1;
  }
  __syncthreads();
  // V^T rows: thread -> (d, 8 consecutive t); 128 d x 8 chunks = 1024 items, 4 per thread
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int item = it * 256 + tid;
    const int d = item >> 3, c = item & 7;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = vt[(c * 8 + e) * 132 + d];
    float* dst = Vt + (bh * 128 + d) * Tp + t0 + c * 8;
    *(float4*)dst = make_float4(x[0], x[1], x[2], x[3]);
    *(float4*)(dst + 4) = make_float4(x[4], x[5], x[6], x[7]);
  }
}
hipError_t launch_qkv_prep_f32x(const float* qkv, const float* qw, const float* kw, const float* rope_cos, const float* rope_sin, float* Q,
                                float* K, float* Vt, int B, int T, int Tp, int H, float eps, hipStream_t st) {
  if (Tp % 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(qkv_prep_f32x_kernel, dim3(Tp / 64, H, B), dim3(256), 0, st, qkv, qw, kw, rope_cos, rope_sin, Q, K, Vt, T, Tp, H, eps);
  return hipGetLastError();
}

hipError_t launch_qkv_prep(const void* qkv, const float* qw, const float* kw, const float* rope_cos,
                           const float* rope_sin, void* Q, void* K, void* Vt, bool bf16, int B, int T, int Tp, int H,
                           float eps, hipStream_t st, int head_dim) {
  dim3 grid(Tp / 64, H, B), block(256);
  if (head_dim == 64) {   // the general form (no 16-byte fast path for 64-wide heads)
    if (bf16)
      hipLaunchKernelGGL((qkv_prep_kernel<bf16_t, 64>), grid, block, 0, st, (const bf16_t*)qkv, qw, kw, rope_cos, rope_sin, (bf16_t*)Q,
                         (bf16_t*)K, (bf16_t*)Vt, T, Tp, H, eps);
    else
      hipLaunchKernelGGL((qkv_prep_kernel<float, 64>), grid, block, 0, st, (const float*)qkv, qw, kw, rope_cos, rope_sin, (float*)Q,
                         (float*)K, (float*)Vt, T, Tp, H, eps);
    return hipGetLastError();
  }
  if (head_dim != 128) return hipErrorInvalidValue;
  if (bf16 && debug_flag(DBG_QKV_PREP_SWROUND) == 1)   // the pre-round-4 rounding: reproducer only (see the kernel)
    hipLaunchKernelGGL(qkv_prep_bf16_kernel<true>, grid, block, 0, st, (const bf16_t*)qkv, qw, kw, rope_cos, rope_sin, (bf16_t*)Q,
                       (bf16_t*)K, (bf16_t*)Vt, T, Tp, H, eps);
  else if (bf16)
    hipLaunchKernelGGL(qkv_prep_bf16_kernel<false>, grid, block, 0, st, (const bf16_t*)qkv, qw, kw, rope_cos, rope_sin, (bf16_t*)Q,
                       (bf16_t*)K, (bf16_t*)Vt, T, Tp, H, eps);
  else
    hipLaunchKernelGGL((qkv_prep_kernel<float, 128>), grid, block, 0, st, (const float*)qkv, qw, kw, rope_cos, rope_sin,
                       (float*)Q, (float*)K, (float*)Vt, T, Tp, H, eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// in-place per-(row, head) RMSNorm (cross-attention k_norm, transformer.py:143-144); wave per (row, head)
// ------------------------------------------------------------------------------------------------
template <typename TA, int HD>
__global__ __launch_bounds__(256) void headnorm_kernel(TA* __restrict__ x, const float* __restrict__ w, long rows,
                                                       long ld, int col0, int H, float eps) {
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= rows * H) return;
  const int lane = threadIdx.x & 63;
  const bool on = lane < HD / 2;   // HD = 64: half the wave sits out
  const long r = item / H;
  const int h = (int)(item % H);
  TA* p = x + r * ld + col0 + h * HD + 2 * lane;
  float a = 0.f, c = 0.f;
  if (on) load2<TA>(p, a, c);
  const float inv = rsqrtf(wave_sum(a * a + c * c) / (float)HD + eps);
  if (on) store2<TA>(p, a * inv * w[2 * lane], c * inv * w[2 * lane + 1]);
}

hipError_t launch_headnorm(void* x, const float* w, bool bf16, int rows, long ld, int col0, int H, float eps,
                           hipStream_t st, int head_dim) {
  const long items = (long)rows * H;
  dim3 grid((unsigned)((items + 3) / 4)), block(256);
  if (head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
  if (bf16 && head_dim == 128)
    hipLaunchKernelGGL((headnorm_kernel<bf16_t, 128>), grid, block, 0, st, (bf16_t*)x, w, (long)rows, ld, col0, H, eps);
  else if (bf16)
    hipLaunchKernelGGL((headnorm_kernel<bf16_t, 64>), grid, block, 0, st, (bf16_t*)x, w, (long)rows, ld, col0, H, eps);
  else if (head_dim == 128)
    hipLaunchKernelGGL((headnorm_kernel<float, 128>), grid, block, 0, st, (float*)x, w, (long)rows, ld, col0, H, eps);
  else
    hipLaunchKernelGGL((headnorm_kernel<float, 64>), grid, block, 0, st, (float*)x, w, (long)rows, ld, col0, H, eps);
  return hipGetLastError();
}

// K halves of all layers' cross-attention key/value projections in one launch: kv_all [rows, L*2D], item =
// (row, layer, head); weight w_all[layer][128]
template <typename TA, int HD>
__global__ __launch_bounds__(256) void headnorm_layers_kernel(TA* __restrict__ x, const float* __restrict__ w_all,
                                                              long rows, int L, int H, float eps) {
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= rows * L * H) return;
  const int lane = threadIdx.x & 63;
  const bool on = lane < HD / 2;
  const int h = (int)(item % H);
  const int l = (int)((item / H) % L);
  const long r = item / ((long)H * L);
  const long D2 = 2L * H * HD;
  TA* p = x + r * (D2 * L) + l * D2 + h * HD + 2 * lane;
  const float* w = w_all + l * HD;
  float a = 0.f, c = 0.f;
  if (on) load2<TA>(p, a, c);
  const float inv = rsqrtf(wave_sum(a * a + c * c) / (float)HD + eps);
  if (on) store2<TA>(p, a * inv * w[2 * lane], c * inv * w[2 * lane + 1]);
}

hipError_t launch_headnorm_layers(void* kv_all, const float* w_all, bool bf16, int rows, int L, int H, float eps,
                                  hipStream_t st, int head_dim) {
  const long items = (long)rows * L * H;
  dim3 grid((unsigned)((items + 3) / 4)), block(256);
  if (head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
  if (bf16 && head_dim == 128)
    hipLaunchKernelGGL((headnorm_layers_kernel<bf16_t, 128>), grid, block, 0, st, (bf16_t*)kv_all, w_all, (long)rows, L, H, eps);
  else if (bf16)
    hipLaunchKernelGGL((headnorm_layers_kernel<bf16_t, 64>), grid, block, 0, st, (bf16_t*)kv_all, w_all, (long)rows, L, H, eps);
  else if (head_dim == 128)
    hipLaunchKernelGGL((headnorm_layers_kernel<float, 128>), grid, block, 0, st, (float*)kv_all, w_all, (long)rows, L, H, eps);
  else
    hipLaunchKernelGGL((headnorm_layers_kernel<float, 64>), grid, block, 0, st, (float*)kv_all, w_all, (long)rows, L, H, eps);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Test aid: leave every CU's LDS full of 0xFFFF words (NaN as bf16 and as fp32).  LDS is not cleared between
// kernels, so a kernel that consumes LDS it never wrote (e.g. an MFMA operand of padding lanes) then produces NaNs
// deterministically instead of depending on which kernel last ran on the CU.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void poison_lds_kernel(unsigned* sink) {
  __shared__ unsigned buf[160 * 1024 / 4];
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) buf[i] = 0xffffffffu;
  __syncthreads();
  if (sink && buf[(threadIdx.x * 37) % (160 * 1024 / 4)] == 0u) sink[0] = 1u;  // keeps the stores alive
}

hipError_t launch_poison_lds(hipStream_t st) {
  hipLaunchKernelGGL(poison_lds_kernel, dim3(1024), dim3(256), 0, st, (unsigned*)nullptr);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// timestep features (reference transformer.py:236-248 and model.py:35-42): cat(cos, sin)(t * freq)
// ------------------------------------------------------------------------------------------------
template <typename TA>
__global__ void time_features_kernel(const float* __restrict__ t, const float* __restrict__ freqs, int fdim,
                                     const float* __restrict__ inv_freq, int D, TA* __restrict__ temb,
                                     float* __restrict__ tsin) {
  const int j = blockIdx.x;
  const float tv = t[j];
  const int hf = fdim / 2, hd = D / 2;
  for (int i = threadIdx.x; i < hf; i += blockDim.x) {
    const float a = tv * freqs[i];
    Elem<TA>::store(temb + (long)j * fdim + i, cosf(a));
    Elem<TA>::store(temb + (long)j * fdim + hf + i, sinf(a));
  }
  for (int i = threadIdx.x; i < hd; i += blockDim.x) {
    const float a = tv * inv_freq[i];
    tsin[(long)j * D + i] = cosf(a);
    tsin[(long)j * D + hd + i] = sinf(a);
  }
}

// dst[0 .. n) = the values, handed over as KERNEL ARGUMENTS: a host -> device copy of a few floats that needs neither pinned host
// memory nor a stream synchronisation to keep a pageable source alive (ode_solve's evaluation times: before, a hipMemcpyAsync +
// hipStreamSynchronize sat between the DAC encode and the first DiT evaluation of every separate())
__global__ void set_floats_kernel(float* __restrict__ dst, const FloatPack v, const int n) {
  const int i = threadIdx.x;
  if (i < n) dst[i] = v.v[i];
}
hipError_t launch_set_floats(float* dst, const float* host_values, int n, hipStream_t st) {
  for (int off = 0; off < n; off += FloatPack::N) {
    FloatPack v;
    const int m = n - off < FloatPack::N ? n - off : FloatPack::N;
    for (int i = 0; i < FloatPack::N; ++i) v.v[i] = i < m ? host_values[off + i] : 0.f;
    hipLaunchKernelGGL(set_floats_kernel, dim3(1), dim3(FloatPack::N), 0, st, dst + off, v, m);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// explicit Runge-Kutta combination (engine.hip solve_rk): out = y0 + scale * (coef0 k0 + coef1 k1 + ...), fp32, float4 per lane.
// The last combination of a step writes y1 over y0, so `y0` and `out` may be the same array: neither is __restrict__ (each lane reads
// its y0 element before it writes the same element, and no lane touches another's).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ode_stage_kernel(const float4* y0, const OdeStageArgs a, const float scale, float4* out,
                                                        const long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 k[4];   // every load first (n_src is uniform: the branches are scalar), then the arithmetic
    k[0] = ((const float4*)a.k[0])[i];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (j < a.n_src) k[j] = ((const float4*)a.k[j])[i];
    const float4 y = y0[i];
    float4 s = make_float4(a.coef[0] * k[0].x, a.coef[0] * k[0].y, a.coef[0] * k[0].z, a.coef[0] * k[0].w);
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (j < a.n_src) {
        s.x += a.coef[j] * k[j].x;
        s.y += a.coef[j] * k[j].y;
        s.z += a.coef[j] * k[j].z;
        s.w += a.coef[j] * k[j].w;
      }
    out[i] = make_float4(y.x + scale * s.x, y.y + scale * s.y, y.z + scale * s.z, y.w + scale * s.w);
  }
}

hipError_t launch_ode_stage(const float* y0, const OdeStageArgs& a, float scale, float* out, long n, hipStream_t st) {
  if (a.n_src < 1 || a.n_src > 4 || n % 4) return hipErrorInvalidValue;
  const long n4 = n / 4;
  long gx = (n4 + 255) / 256;
  if (gx > 2048) gx = 2048;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(ode_stage_kernel, dim3((unsigned)gx), dim3(256), 0, st, (const float4*)y0, a, scale, (float4*)out, n4);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// adaptive solve with per-row step control (engine.hip Engine::ode_solve_adaptive).  blockIdx.y is the row everywhere, so a
// row's status and step are uniform over a block: the branches on them are scalar.
// ------------------------------------------------------------------------------------------------
// out = y + h[r] * sum_j coef[j] k[j] for running rows; a finished or failed row is copied through WITHOUT reading its K (which may hold
// anything, NaN included: a predicate, not a multiplication by zero).  out may be y itself, never a k.
__global__ __launch_bounds__(256) void ode_stage_rows_kernel(const float4* y, const OdeSrcArgs a, const OdeRowCtl* __restrict__ ctl,
                                                             float4* out, const long row4) {
  const int r = blockIdx.y;
  const bool run = ctl[r].status == ODE_ROW_RUNNING;
  const float h = ctl[r].h;
  const long base = (long)r * row4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < row4; i += (long)gridDim.x * 256) {
    const float4 v = y[base + i];
    if (!run) {
      out[base + i] = v;
      continue;
    }
    float4 k[kOdeMaxSrc];
#pragma unroll
    for (int j = 0; j < kOdeMaxSrc; ++j)
      if (j < a.n_src) k[j] = ((const float4*)a.k[j])[base + i];
    float4 s = make_float4(a.coef[0] * k[0].x, a.coef[0] * k[0].y, a.coef[0] * k[0].z, a.coef[0] * k[0].w);
#pragma unroll
    for (int j = 1; j < kOdeMaxSrc; ++j)
      if (j < a.n_src) {
        s.x += a.coef[j] * k[j].x;
        s.y += a.coef[j] * k[j].y;
        s.z += a.coef[j] * k[j].z;
        s.w += a.coef[j] * k[j].w;
      }
    out[base + i] = make_float4(v.x + h * s.x, v.y + h * s.y, v.z + h * s.z, v.w + h * s.w);
  }
}

hipError_t launch_ode_stage_rows(const float* y, const OdeSrcArgs& a, const OdeRowCtl* ctl, float* out, int rows, long row_elems,
                                 hipStream_t st) {
  if (a.n_src < 1 || a.n_src > kOdeMaxSrc || rows < 1 || rows > 65535 || row_elems < 4 || row_elems % 4) return hipErrorInvalidValue;
  const long row4 = row_elems / 4;
  long gx = (row4 + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(ode_stage_rows_kernel, dim3((unsigned)gx, (unsigned)rows), dim3(256), 0, st, (const float4*)y, a, ctl, (float4*)out,
                     row4);
  return hipGetLastError();
}

// The sum of squares of one chunk of one row's scaled error, in an order that depends on nothing but the element's place in the row:
// block (c, r) owns elements [c * kOdeChunk, (c + 1) * kOdeChunk) of row r, lane l adds its 16 elements in index order (float4 number
// l, l + 256, l + 512, l + 768 of the chunk), the 256 lane sums meet in a fixed binary tree in LDS, and the chunk's sum is written to
// partials[r, c] for ode_control_kernel to add in chunk order.  No atomics.  An element of a padding frame adds nothing (a predicate),
// so chunks behind a row's valid prefix hold +0 and a larger padded frame count only appends zeros to a sum of non-negative terms:
// the row's norm has the same bits alone, among other rows and in a longer batch.
__global__ __launch_bounds__(256) void ode_error_kernel(const float4* __restrict__ y, const float4* __restrict__ ynew, const OdeSrcArgs a,
                                                        const OdeRowCtl* __restrict__ ctl, const unsigned char* __restrict__ mask,
                                                        const float rtol, const float atol, const int use_h,
                                                        float* __restrict__ partials, const int frames, const int chan4) {
  __shared__ float red[256];
  const int r = blockIdx.y, c = blockIdx.x, l = threadIdx.x;
  const long row4 = (long)frames * chan4;
  float sum = 0.f;
  if (ctl[r].status == ODE_ROW_RUNNING) {
    const float m = use_h ? ctl[r].h : 1.f;
    const long base = (long)r * row4;
#pragma unroll
    for (int it = 0; it < kOdeChunk / 1024; ++it) {
      const long i = (long)c * (kOdeChunk / 4) + it * 256 + l;
      if (i >= row4) continue;
      if (mask && !mask[(long)r * frames + i / chan4]) continue;
      float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < kOdeMaxSrc; ++j)
        if (j < a.n_src) {
          const float4 k = ((const float4*)a.k[j])[base + i];
          e.x += a.coef[j] * k.x;
          e.y += a.coef[j] * k.y;
          e.z += a.coef[j] * k.z;
          e.w += a.coef[j] * k.w;
        }
      const float4 v = y[base + i];
      float4 w = v;
      if (ynew) w = ynew[base + i];
      const float qx = m * e.x / (atol + rtol * fmaxf(fabsf(v.x), fabsf(w.x)));
      const float qy = m * e.y / (atol + rtol * fmaxf(fabsf(v.y), fabsf(w.y)));
      const float qz = m * e.z / (atol + rtol * fmaxf(fabsf(v.z), fabsf(w.z)));
      const float qw = m * e.w / (atol + rtol * fmaxf(fabsf(v.w), fabsf(w.w)));
      sum += qx * qx;
      sum += qy * qy;
      sum += qz * qz;
      sum += qw * qw;
    }
  }
  red[l] = sum;
  for (int o = 128; o > 0; o >>= 1) {
    __syncthreads();
    if (l < o) red[l] += red[l + o];
  }
  if (l == 0) partials[(long)r * gridDim.x + c] = red[0];
}

hipError_t launch_ode_error(const float* y, const float* ynew, const OdeSrcArgs& a, const OdeRowCtl* ctl, const unsigned char* mask,
                            float rtol, float atol, int use_h, float* partials, int rows, int frames, int channels, hipStream_t st) {
  if (a.n_src < 1 || a.n_src > kOdeMaxSrc || rows < 1 || rows > 65535 || frames < 1 || channels < 4 || channels % 4)
    return hipErrorInvalidValue;
  const long chunks = ((long)frames * channels + kOdeChunk - 1) / kOdeChunk;
  hipLaunchKernelGGL(ode_error_kernel, dim3((unsigned)chunks, (unsigned)rows), dim3(256), 0, st, (const float4*)y, (const float4*)ynew, a,
                     ctl, mask, rtol, atol, use_h, partials, frames, channels / 4);
  return hipGetLastError();
}

// The controller: scipy's RungeKutta._step_impl (max_step = inf) and select_initial_step, one lane per row, fp32 throughout.
// Contraction is off in the bookkeeping: t, h and the stage times are the separately rounded products and sums that a float32
// restatement computes; powf is the one operation that may differ from it in the last place.
__device__ inline void ode_row_begin_trial(OdeRowCtl& c, const OdeControlArgs& a, float* times, const int rows, const int r) {
#pragma clang fp contract(off)
  if (c.accepted + c.rejected >= a.max_num_steps) {
    c.status = ODE_ROW_MAX_STEPS;
    return;
  }
  const float min_step = 10.f * (nextafterf(c.t, INFINITY) - c.t);
  if (!c.step_rejected) {
    if (c.h_abs < min_step) c.h_abs = min_step;
  } else if (c.h_abs < min_step) {
    c.status = ODE_ROW_STEP_UNDERFLOW;
    return;
  }
  float t_new = c.t + c.h_abs;
  if (t_new - a.t1 > 0.f) t_new = a.t1;
  c.t_new = t_new;
  c.h = t_new - c.t;
  for (int i = 0; i < a.n_times; ++i) times[(long)i * rows + r] = c.t + a.c[i] * c.h;
}

// what a running row does with the sums of its norm partials (`ss`; `ss_b`: INIT1's second norm): the two halves of the initial-step
// rule, or the accept / reject decision and the next trial.  The times of the next trial go to column r of the table.
__device__ inline void ode_row_decide(OdeRowCtl& c, const int mode, const OdeControlArgs& a, const float ss, const float ss_b,
                                      float* times, const int rows, const int r) {
#pragma clang fp contract(off)
  const float n = (float)(c.n_valid > 0 ? c.n_valid : 1);
  const float norm = sqrtf(ss / n);
  if (mode == ODE_CTL_INIT1) {   // d0 = |y0 / scale|, d1 = |f0 / scale|: the explicit-Euler probe step h0
    const float d0 = norm, d1 = sqrtf(ss_b / n);
    float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
    h0 = fminf(h0, a.t1 - a.t0);
    c.d1 = d1;
    c.h0 = c.h = h0;
    times[rows + r] = a.t0 + h0;
  } else if (mode == ODE_CTL_INIT2) {   // d2 = |(f1 - f0) / scale| / h0
    const float d2 = norm / c.h0;
    const float h1 = (c.d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, c.h0 * 1e-3f)
                                                      : powf(0.01f / fmaxf(c.d1, d2), 1.f / (float)(a.order + 1));
    c.h_abs = fminf(fminf(100.f * c.h0, h1), a.t1 - a.t0);
    ode_row_begin_trial(c, a, times, rows, r);
  } else {
    const float expo = -1.f / (float)(a.order + 1);
    c.err = norm;
    c.h_abs = c.h;
    if (norm < 1.f) {
      float factor = norm == 0.f ? a.ifactor : fminf(a.ifactor, a.safety * powf(norm, expo));
      if (c.step_rejected) factor = fminf(1.f, factor);
      c.h_abs *= factor;
      c.h_prev = c.h;
      c.t = c.t_new;
      c.accepted += 1;
      c.accepted_now = 1;
      c.step_rejected = 0;
      if (c.t - a.t1 >= 0.f) c.status = ODE_ROW_FINISHED;
    } else {   // (a NaN norm lands here: fmaxf drops it and the step shrinks by dfactor until it underflows)
      c.h_abs *= fmaxf(a.dfactor, a.safety * powf(norm, expo));
      c.rejected += 1;
      c.accepted_now = 0;
      c.step_rejected = 1;
    }
    if (c.status == ODE_ROW_RUNNING) ode_row_begin_trial(c, a, times, rows, r);
  }
  if (c.status != ODE_ROW_RUNNING)   // a row that stops rides along at its own time
    for (int i = 0; i < a.n_times; ++i) times[(long)i * rows + r] = c.t;
}

// a row (or a group's leader row) at the start of a solve; `valid` = the frames its norms count
__device__ inline void ode_row_reset(OdeRowCtl& c, const OdeControlArgs& a, const int valid, const int channels, float* times,
                                     const int rows, const int r) {
  c = OdeRowCtl{};
  c.t = c.t_new = a.t0;
  c.n_valid = valid * channels;
  for (int i = 0; i < a.n_times; ++i) times[(long)i * rows + r] = a.t0;
  if (a.first_step > 0.f) {
    c.h_abs = a.first_step;
    ode_row_begin_trial(c, a, times, rows, r);
  }
}

__global__ __launch_bounds__(256) void ode_control_kernel(OdeRowCtl* ctl, const int mode, const OdeControlArgs a,
                                                          const float* __restrict__ partials, const float* __restrict__ partials_b,
                                                          const int chunks, const unsigned char* __restrict__ mask, const int frames,
                                                          const int channels, float* times, int* active, const int rows) {
#pragma clang fp contract(off)
  __shared__ int running[256];
  int mine = 0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    OdeRowCtl c = ctl[r];
    if (mode == ODE_CTL_RESET) {
      int valid = frames;
      if (mask) {
        valid = 0;
        for (int f = 0; f < frames; ++f) valid += mask[(long)r * frames + f] != 0;
      }
      ode_row_reset(c, a, valid, channels, times, rows, r);
    } else if (c.status == ODE_ROW_RUNNING) {
      float ss = 0.f, ss_b = 0.f;
      for (int k = 0; k < chunks; ++k) ss += partials[(long)r * chunks + k];
      if (mode == ODE_CTL_INIT1)
        for (int k = 0; k < chunks; ++k) ss_b += partials_b[(long)r * chunks + k];
      ode_row_decide(c, mode, a, ss, ss_b, times, rows, r);
    } else {
      c.accepted_now = 0;
    }
    ctl[r] = c;
    mine += c.status == ODE_ROW_RUNNING;
  }
  running[threadIdx.x] = mine;
  for (int o = 128; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) running[threadIdx.x] += running[threadIdx.x + o];
  }
  if (threadIdx.x == 0) *active = running[0];
}

// Step control per GROUP of rows (the window rows of one clip and candidate in a windowed solve): one lane per
// group.  groups [n_groups, 3] i32 = first row, row count, row stride; null: every row is a group of its own, which is
// ode_control_kernel's arithmetic.  A group is ONE integration: its norm is the sum of its rows' partials - rows in window order,
// chunks in order within a row, one accumulator, no atomics - over n_valid = the masked frames of all its rows * channels (`mask`
// is the ownership mask there: every frame of the clip is counted in exactly one row), and every row of the group receives the
// same control block and the same column of the time table.  A row index outside [0, rows) is absent: a bad table groups wrong rows
// but never reaches outside the arrays.  *active = rows (not groups) still running.
__global__ __launch_bounds__(256) void ode_control_groups_kernel(OdeRowCtl* ctl, const int mode, const OdeControlArgs a,
                                                                 const float* __restrict__ partials,
                                                                 const float* __restrict__ partials_b, const int chunks,
                                                                 const unsigned char* __restrict__ mask, const int frames,
                                                                 const int channels, float* times, int* active, const int rows,
                                                                 const int* __restrict__ groups, const int n_groups) {
#pragma clang fp contract(off)
  __shared__ int running[256];
  int mine = 0;
  for (int g = threadIdx.x; g < n_groups; g += 256) {
    const int first = groups ? groups[3 * g] : g;
    int count = groups ? groups[3 * g + 1] : 1;
    const int stride = groups ? groups[3 * g + 2] : 1;
    if (count > rows) count = rows;
    auto row_of = [&](int w) {   // -1: absent
      const long r = (long)first + (long)w * stride;
      return r >= 0 && r < rows ? (int)r : -1;
    };
    int lead = -1, present = 0;
    for (int w = 0; w < count; ++w) {
      const int r = row_of(w);
      if (r < 0) continue;
      if (lead < 0) lead = r;
      ++present;
    }
    if (lead < 0) continue;
    OdeRowCtl c = ctl[lead];
    if (mode == ODE_CTL_RESET) {
      int valid = 0;
      for (int w = 0; w < count; ++w) {
        const int r = row_of(w);
        if (r < 0) continue;
        if (mask) {
          for (int f = 0; f < frames; ++f) valid += mask[(long)r * frames + f] != 0;
        } else {
          valid += frames;
        }
      }
      ode_row_reset(c, a, valid, channels, times, rows, lead);
    } else if (c.status == ODE_ROW_RUNNING) {
      float ss = 0.f, ss_b = 0.f;
      for (int w = 0; w < count; ++w) {
        const int r = row_of(w);
        if (r < 0) continue;
        for (int k = 0; k < chunks; ++k) ss += partials[(long)r * chunks + k];
      }
      if (mode == ODE_CTL_INIT1)
        for (int w = 0; w < count; ++w) {
          const int r = row_of(w);
          if (r < 0) continue;
          for (int k = 0; k < chunks; ++k) ss_b += partials_b[(long)r * chunks + k];
        }
      ode_row_decide(c, mode, a, ss, ss_b, times, rows, lead);
    } else {
      c.accepted_now = 0;
    }
    for (int w = 0; w < count; ++w) {   // the leader's block and its column of the time table, to every row of the group
      const int r = row_of(w);
      if (r < 0) continue;
      ctl[r] = c;
      if (r != lead)
        for (int i = 0; i < a.n_times; ++i) times[(long)i * rows + r] = times[(long)i * rows + lead];
    }
    mine += c.status == ODE_ROW_RUNNING ? present : 0;
  }
  running[threadIdx.x] = mine;
  for (int o = 128; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) running[threadIdx.x] += running[threadIdx.x + o];
  }
  if (threadIdx.x == 0) *active = running[0];
}

hipError_t launch_ode_control(OdeRowCtl* ctl, int mode, const OdeControlArgs& a, const float* partials, const float* partials_b,
                              int chunks, const unsigned char* mask, int frames, int channels, float* times, int* active, int rows,
                              hipStream_t st) {
  if (rows < 1 || mode < ODE_CTL_RESET || mode > ODE_CTL_STEP || a.n_times < 2 || a.n_times > kOdeMaxSrc) return hipErrorInvalidValue;
  if (mode != ODE_CTL_RESET && (!partials || chunks < 1)) return hipErrorInvalidValue;
  if (mode == ODE_CTL_INIT1 && !partials_b) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ode_control_kernel, dim3(1), dim3(256), 0, st, ctl, mode, a, partials, partials_b, chunks, mask, frames, channels,
                     times, active, rows);
  return hipGetLastError();
}

hipError_t launch_ode_control_groups(OdeRowCtl* ctl, int mode, const OdeControlArgs& a, const float* partials, const float* partials_b,
                                     int chunks, const unsigned char* mask, int frames, int channels, float* times, int* active,
                                     int rows, const int* groups, int n_groups, hipStream_t st) {
  if (rows < 1 || mode < ODE_CTL_RESET || mode > ODE_CTL_STEP || a.n_times < 2 || a.n_times > kOdeMaxSrc) return hipErrorInvalidValue;
  if (mode != ODE_CTL_RESET && (!partials || chunks < 1)) return hipErrorInvalidValue;
  if (mode == ODE_CTL_INIT1 && !partials_b) return hipErrorInvalidValue;
  if (groups ? n_groups < 1 : n_groups != rows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ode_control_groups_kernel, dim3(1), dim3(256), 0, st, ctl, mode, a, partials, partials_b, chunks, mask, frames,
                     channels, times, active, rows, groups, n_groups);
  return hipGetLastError();
}

// accepted rows: y <- y_new and (first same as last) K[0] <- K[last]; the other rows keep both
__global__ __launch_bounds__(256) void ode_commit_kernel(float4* __restrict__ y, const float4* __restrict__ ynew,
                                                         float4* __restrict__ k_first, const float4* __restrict__ k_last,
                                                         const OdeRowCtl* __restrict__ ctl, const long row4) {
  const int r = blockIdx.y;
  if (!ctl[r].accepted_now) return;
  const long base = (long)r * row4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < row4; i += (long)gridDim.x * 256) {
    y[base + i] = ynew[base + i];
    k_first[base + i] = k_last[base + i];
  }
}

hipError_t launch_ode_commit(float* y, const float* ynew, float* k_first, const float* k_last, const OdeRowCtl* ctl, int rows,
                             long row_elems, hipStream_t st) {
  if (rows < 1 || rows > 65535 || row_elems < 4 || row_elems % 4) return hipErrorInvalidValue;
  const long row4 = row_elems / 4;
  long gx = (row4 + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(ode_commit_kernel, dim3((unsigned)gx, (unsigned)rows), dim3(256), 0, st, (float4*)y, (const float4*)ynew,
                     (float4*)k_first, (const float4*)k_last, ctl, row4);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// windowed solve of long clips (engine.hip eval_field): the last O frames of a window row and the first O frames
// of its successor row describe the same frames of the clip; after every field evaluation both are replaced by their cross-fade
// v = p + a_j (q - p), a_j = (j + 1) / (O + 1), in place, float4 per lane.  One lane reads both elements of a pair and writes the same
// value to both, so no two lanes touch the same address: the tail of a row is frames [W - O, W), the head [0, O), disjoint because
// O <= W / 2, and a row is the successor of at most one row (the table is the caller's; an entry outside [0, rows) or equal to its own
// index is treated as "no successor", so a bad table blends wrong rows but never reaches outside the tensor).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_blend_kernel(float* out, const int* __restrict__ next_row, const int rows, const int W,
                                                           const int O, const int n4, const long total) {
  const float den = (float)(O + 1);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c4 = (int)(i % n4);
    const long t = i / n4;
    const int j = (int)(t % O), r = (int)(t / O);
    const int s = next_row[r];
    if (s < 0 || s >= rows || s == r) continue;
    float4* const pp = (float4*)out + ((long)r * W + (W - O) + j) * n4 + c4;
    float4* const pq = (float4*)out + ((long)s * W + j) * n4 + c4;
    const float4 p = *pp, q = *pq;
    const float a = (float)(j + 1) / den;   // the fp32 weight (a divide per float4 pair is free next to the four memory accesses)
    const float4 v = make_float4(fmaf(a, q.x - p.x, p.x), fmaf(a, q.y - p.y, p.y), fmaf(a, q.z - p.z, p.z), fmaf(a, q.w - p.w, p.w));
    *pp = v;
    *pq = v;
  }
}

hipError_t launch_window_blend(float* out, const int* next_row, int rows, int W, int O, int C2, hipStream_t st) {
  if (!out || !next_row || rows < 1 || O < 1 || O > W / 2 || C2 < 4 || C2 % 4) return hipErrorInvalidValue;
  const int n4 = C2 / 4;
  const long total = (long)rows * O * n4;
  long gx = (total + 255) / 256;
  if (gx > 2048) gx = 2048;
  hipLaunchKernelGGL(window_blend_kernel, dim3((unsigned)gx), dim3(256), 0, st, out, next_row, rows, W, O, n4, total);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// seeded noise of separate(seed=...) (tests/noise_ref.py is the statement).  One lane per quad of four
// channels: one Philox4x32-10 call (Random123's constants; the high product as a 64-bit multiply), two Box-Muller pairs in plain fp32,
// one float4 store - consecutive lanes write consecutive 16 bytes of a row.  The counter is (t * Q + q, candidate, clip id lo, hi), the
// key the seed: a value depends on nothing else, so padding, batch composition, candidate count and the split into launches leave
// every bit alone.  Both uniforms are exact in fp32: u_a = ((x >> 8) + 1) 2^-24 in (0, 1] (the logarithm's; 1 gives r = 0),
// u_b = (x >> 8) 2^-24 in [0, 1) (the angle's).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x, p1 = (unsigned long long)0xCD9E8D57u * c.z;
    c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ float2 box_muller(unsigned xa, unsigned xb) {
  const float ua = (float)((xa >> 8) + 1u) * 0x1p-24f, ub = (float)(xb >> 8) * 0x1p-24f;   // 24-bit integers: both exact
  const float r = sqrtf(-2.f * logf(ua));
  const float th = 6.28318530717958647692f * ub;
  return make_float2(r * cosf(th), r * sinf(th));
}

// per_stream = frames * Q quads of one (clip, candidate) row, <= 2^32: the quad's index inside its row is counter word 0
__global__ __launch_bounds__(256) void noise_rows_kernel(float4* __restrict__ out, const NoiseClipPack ids, const int candidates,
                                                         const unsigned long long per_stream, const long total, const unsigned k0,
                                                         const unsigned k1) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const unsigned long long row = (unsigned long long)i / per_stream;   // b * candidates + c of this launch's clips
    const unsigned w0 = (unsigned)((unsigned long long)i - row * per_stream);
    const unsigned b = (unsigned)(row / (unsigned)candidates), c = (unsigned)(row % (unsigned)candidates);
    const unsigned long long id = (unsigned long long)ids.v[b];
    const uint4 x = philox4x32_10(make_uint4(w0, c, (unsigned)id, (unsigned)(id >> 32)), k0, k1);
    const float2 z01 = box_muller(x.x, x.y), z23 = box_muller(x.z, x.w);
    out[i] = make_float4(z01.x, z01.y, z23.x, z23.y);
  }
}

hipError_t launch_noise_rows(float* out, int clips, int candidates, int frames, int channels, unsigned long long seed,
                             const long long* clip_ids, hipStream_t st) {
  if (!out || !clip_ids || clips < 1 || candidates < 1 || frames < 1 || channels < 4 || channels % 4) return hipErrorInvalidValue;
  const unsigned long long per_stream = (unsigned long long)frames * (unsigned)(channels / 4);
  // counter word 0 holds the quad index of a row; 64 clips of a launch stay far inside a signed 64-bit index
  if (per_stream > (1ull << 32) || (unsigned long long)candidates * per_stream > (1ull << 56)) return hipErrorInvalidValue;
  for (int off = 0; off < clips; off += NoiseClipPack::N) {
    NoiseClipPack ids;
    const int m = clips - off < NoiseClipPack::N ? clips - off : NoiseClipPack::N;
    for (int i = 0; i < NoiseClipPack::N; ++i) ids.v[i] = i < m ? clip_ids[off + i] : 0;
    const long total = (long)((unsigned long long)m * candidates * per_stream);
    long gx = (total + 255) / 256;
    if (gx > kNoiseGridCap) gx = kNoiseGridCap;
    hipLaunchKernelGGL(noise_rows_kernel, dim3((unsigned)gx), dim3(256), 0, st,
                       (float4*)out + (unsigned long long)off * candidates * per_stream, ids, candidates, per_stream, total,
                       (unsigned)seed, (unsigned)(seed >> 32));
  }
  return hipGetLastError();
}

hipError_t launch_time_features(const float* t, int nt, const float* freqs, int fdim, const float* inv_freq, int D,
                                void* temb, float* tsin, bool bf16, hipStream_t st) {
  if (bf16)
    hipLaunchKernelGGL(time_features_kernel<bf16_t>, dim3(nt), dim3(256), 0, st, t, freqs, fdim, inv_freq, D,
                       (bf16_t*)temb, tsin);
  else
    hipLaunchKernelGGL(time_features_kernel<float>, dim3(nt), dim3(256), 0, st, t, freqs, fdim, inv_freq, D,
                       (float*)temb, tsin);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// memory = memory_proj(text) + timestep_emb   (reference model.py:170-172) -> AT operand
// ------------------------------------------------------------------------------------------------
template <typename TA>
__global__ __launch_bounds__(256) void add_rowvec_kernel(const float* __restrict__ x, const float* __restrict__ vec,
                                                         long vec_ld, TA* __restrict__ out, long rows, int D,
                                                         int rows_per_b) {
  const int n4 = D >> 2;
  const long total = rows * n4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / n4;
    const int c4 = (int)(i % n4);
    float4 v = ((const float4*)x)[i];
    float4 a = *(const float4*)(vec + (r / rows_per_b) * vec_ld + 4 * c4);
    store4<TA>(out + 4 * i, v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
  }
}

hipError_t launch_add_rowvec(const float* x, const float* vec, long vec_ld, void* out, bool bf16, int rows, int D,
                             int rows_per_b, hipStream_t st) {
  long total = (long)rows * (D / 4);
  int gx = (int)((total + 255) / 256);
  if (gx > 2048) gx = 2048;
  if (bf16)
    hipLaunchKernelGGL(add_rowvec_kernel<bf16_t>, dim3(gx), dim3(256), 0, st, x, vec, vec_ld, (bf16_t*)out,
                       (long)rows, D, rows_per_b);
  else
    hipLaunchKernelGGL(add_rowvec_kernel<float>, dim3(gx), dim3(256), 0, st, x, vec, vec_ld, (float*)out, (long)rows,
                       D, rows_per_b);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// anchor embedding gather (reference model.py:61: embed(anchor_ids.gather(1, anchor_alignment)))
// ------------------------------------------------------------------------------------------------
template <typename TA>
__global__ void anchor_gather_kernel(const float* __restrict__ emb, const long* __restrict__ ids, int n_ids,
                                     const long* __restrict__ align, TA* __restrict__ out, int T, int E, int vocab) {
  const long r = blockIdx.x;  // row b*T + t
  const long b = r / T;
  // indices arrive through the public ABI: out-of-range values are clamped here so that the kernel never reads outside
  // its tables (the host classes reject them with the reference's exception type before they get this far)
  long slot = align[r];
  slot = slot < 0 ? 0 : (slot >= n_ids ? n_ids - 1 : slot);
  long tok = ids[b * n_ids + slot];
  tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
  for (int i = threadIdx.x; i < E; i += blockDim.x) Elem<TA>::store(out + r * E + i, emb[tok * E + i]);
}

hipError_t launch_anchor_gather(const float* emb, const long* ids, int n_ids, const long* align, void* out, bool bf16,
                                int B, int T, int E, int vocab, hipStream_t st) {
  if (bf16)
    hipLaunchKernelGGL(anchor_gather_kernel<bf16_t>, dim3(B * T), dim3(64), 0, st, emb, ids, n_ids, align,
                       (bf16_t*)out, T, E, vocab);
  else
    hipLaunchKernelGGL(anchor_gather_kernel<float>, dim3(B * T), dim3(64), 0, st, emb, ids, n_ids, align, (float*)out,
                       T, E, vocab);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// fp32 -> AT copy into a (halo-padded, channel-padded) channels-last buffer
// ------------------------------------------------------------------------------------------------
template <typename TA>
__global__ __launch_bounds__(256) void to_act_kernel(const float* __restrict__ in, long in_bstride, long in_ld,
                                                     int in_col0, TA* __restrict__ out, long out_bstride, long T,
                                                     int C_in, int C_out, int halo) {
  const int b = blockIdx.y;
  const long total = T * C_out;
  const float* ib = in + (long)b * in_bstride + in_col0;
  TA* ob = out + (long)b * out_bstride + (long)halo * C_out;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long t = i / C_out;
    const int c = (int)(i % C_out);
    Elem<TA>::store(ob + i, c < C_in ? ib[t * in_ld + c] : 0.f);
  }
}

hipError_t launch_to_act(const float* in, long in_bstride, long in_ld, int in_col0, void* out, long out_bstride,
                         bool bf16, int B, long T, int C_in, int C_out, int halo, hipStream_t st) {
  if (out_bstride == 0) out_bstride = (T + 2L * halo) * C_out;
  long total = T * C_out;
  int gx = (int)((total + 255) / 256);
  if (gx > 1024) gx = 1024;
  if (bf16)
    hipLaunchKernelGGL(to_act_kernel<bf16_t>, dim3(gx, B), dim3(256), 0, st, in, in_bstride, in_ld, in_col0,
                       (bf16_t*)out, out_bstride, T, C_in, C_out, halo);
  else
    hipLaunchKernelGGL(to_act_kernel<float>, dim3(gx, B), dim3(256), 0, st, in, in_bstride, in_ld, in_col0,
                       (float*)out, out_bstride, T, C_in, C_out, halo);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// An fp32 activation row x[K] into the compensated 16-bit row [lo | hi | hi] of 3K elements (the split and its clamp: common.h
// split_h16x2).  One thread = 8 consecutive elements: two 16-byte loads, three 16-byte stores.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ x, long ldx, bf16_t* __restrict__ out,
                                                     long chunks, int cpr, int K) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long)gridDim.x * 256) {
    const long m = i / cpr;
    const int c = (int)(i - m * cpr) * 8;
    const float* src = x + m * ldx + c;
    const float4 a = *(const float4*)src, b = *(const float4*)(src + 4);
    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const H16Split s = split_h16x2(v[2 * e], v[2 * e + 1]);
      hi[e] = s.hi;
      lo[e] = s.lo;
    }
    bf16_t* dst = out + m * (3L * K) + c;
    *(uint4*)dst = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    *(uint4*)(dst + K) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *(uint4*)(dst + 2L * K) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  }
}

hipError_t launch_split3(const float* x, long ldx, void* out, long M, int K, hipStream_t st) {
  if (K % 8 || ldx % 4 || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return hipErrorInvalidValue;
  const int cpr = K / 8;
  const long chunks = M * cpr;
  long gx = (chunks + 255) / 256;
  if (gx > 8192) gx = 8192;
  hipLaunchKernelGGL(split3_kernel, dim3((unsigned)gx), dim3(256), 0, st, x, ldx, (bf16_t*)out, chunks, cpr, K);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// out[b][e] = act(in[b][e]; alpha[e % chan]) over `count` contiguous fp32 values per batch item (in-place allowed): the activation
// of a codec convolution whose multiply ran as a compensated 16-bit launch (engine.hip gemm_codec_x3) - the same snake_f / tanhf
// expressions as the fp32 convolution kernel's epilogue (gemm.hip), applied to its raw fp32 result
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void act_flat_kernel(const float* __restrict__ in, long in_bstride, float* __restrict__ out,
                                                       long out_bstride, long count, int chan, int act, const float* __restrict__ alpha) {
  const float* ib = in + (long)blockIdx.y * in_bstride;
  float* ob = out + (long)blockIdx.y * out_bstride;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < count; i += (long)gridDim.x * 1024) {
    const float4 v = *(const float4*)(ib + i);
    const int c = (int)(i % chan);
    float4 r;
    if (act == ACT_SNAKE) {
      const float4 al = *(const float4*)(alpha + c);
      r = make_float4(snake_f(v.x, al.x), snake_f(v.y, al.y), snake_f(v.z, al.z), snake_f(v.w, al.w));
    } else if (act == ACT_TANH) {
      r = make_float4(tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(v.w));
    } else if (act == ACT_SILU) {
      r = make_float4(silu_f(v.x), silu_f(v.y), silu_f(v.z), silu_f(v.w));
    } else {
      r = v;
    }
    *(float4*)(ob + i) = r;
  }
}
hipError_t launch_act_flat(const float* in, long in_bstride, float* out, long out_bstride, int items, long count, int chan, int act,
                           const float* alpha, hipStream_t st) {
  if (count % 4 || chan % 4 || in_bstride % 4 || out_bstride % 4 || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) ||
      (act == ACT_SNAKE && (!alpha || ((uintptr_t)alpha & 15))))
    return hipErrorInvalidValue;
  long gx = (count / 4 + 255) / 256;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(act_flat_kernel, dim3((unsigned)gx, items), dim3(256), 0, st, in, in_bstride, out, out_bstride, count, chan, act, alpha);
  return hipGetLastError();
}

template <typename TA>
__global__ void zero_halo_kernel(TA* __restrict__ buf, long T, int C, int halo) {
  const int b = blockIdx.y;
  TA* base = buf + (long)b * (T + 2L * halo) * C;
  const long n = (long)halo * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    Elem<TA>::store(base + i, 0.f);
    Elem<TA>::store(base + (T + halo) * C + i, 0.f);
  }
}

hipError_t launch_zero_halo(void* buf, bool bf16, int B, long T, int C, int halo, hipStream_t st) {
  long n = (long)halo * C;
  int gx = (int)((n + 255) / 256);
  if (gx > 64) gx = 64;
  if (bf16)
    hipLaunchKernelGGL(zero_halo_kernel<bf16_t>, dim3(gx, B), dim3(256), 0, st, (bf16_t*)buf, T, C, halo);
  else
    hipLaunchKernelGGL(zero_halo_kernel<float>, dim3(gx, B), dim3(256), 0, st, (float*)buf, T, C, halo);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Audio front end (samaudio.h samaudio_op_resample): one PCM clip -> its mono mix at the model's rate, right
// padded with zeros.  A workgroup owns `tile` consecutive outputs.  Its lanes are consecutive j, so consecutive phases p: the
// tap-major bank is read at consecutive addresses.  The input window the tile's taps reach is converted and mixed to mono ONCE into
// LDS (the launcher sizes `tile` so that it fits for a well-formed bank); a tile whose window does not fit - a ratio with more than
// ~8000 inputs per 256 outputs, or a `first` table that jumps about - reads the same mono values straight from memory, so both
// paths give the same bits.  Output j is one fma chain over its K taps in ascending d, whoever computes it.
// ------------------------------------------------------------------------------------------------
constexpr int kResampleWindow = 8192;    // fp32 input samples of LDS per workgroup (32 KiB: four workgroups per CU)
constexpr int kResampleTileMax = 2048;   // outputs per workgroup (8 per thread)

__device__ __forceinline__ float pcm_value(float v) { return v; }
__device__ __forceinline__ float pcm_value(short v) { return (float)v * (1.f / 32768.f); }

// mean over the channels of input sample i (0 outside the clip): channel 0 first, fp32, one division
template <typename T>
__device__ __forceinline__ float pcm_mono(const T* __restrict__ pcm, int C, long samples, long ch_stride, long s_stride, long i) {
  if (i < 0 || i >= samples) return 0.f;
  const T* p = pcm + i * s_stride;
  float s = pcm_value(p[0]);
  if (C == 1) return s;
  for (int c = 1; c < C; ++c) s += pcm_value(p[c * ch_stride]);
  return s / (float)C;
}

template <typename T>
__global__ __launch_bounds__(256) void resample_mix_kernel(const T* __restrict__ pcm, int C, long samples, long ch_stride,
                                                           long s_stride, const float* __restrict__ taps,
                                                           const int* __restrict__ first, int n, int o, int K,
                                                           float* __restrict__ out, long out_len, long out_capacity, int tile) {
  __shared__ float win[kResampleWindow];
  __shared__ long long red_lo[256], red_hi[256];
  const int tid = threadIdx.x;
  const long j0 = (long)blockIdx.x * tile;
  const long room = out_capacity - j0, left = out_len - j0;
  const int nout = room < tile ? (int)room : tile;                       // outputs this workgroup writes
  const int nlive = left <= 0 ? 0 : (left < nout ? (int)left : nout);    // ... of which this many are samples, the rest padding
  const long f0 = j0 / n;                                                // j = j0 + r: f = f0 + (p0 + r) / n, p = (p0 + r) % n
  const unsigned p0 = (unsigned)(j0 - f0 * n);
  bool in_lds = false;
  long lo = 0;
  if (nlive > 0) {   // (uniform over the workgroup)
    // the window: from the first tap of any live output to the last one
    long long mn = 0x7fffffffffffffffLL, mx = -0x7fffffffffffffffLL;
    for (int r = tid; r < nlive; r += 256) {
      const unsigned q = p0 + (unsigned)r, df = q / (unsigned)n, p = q - df * (unsigned)n;
      const long long s = (f0 + df) * (long long)o + first[p];
      mn = s < mn ? s : mn;
      mx = s + (K - 1) > mx ? s + (K - 1) : mx;
    }
    red_lo[tid] = mn;
    red_hi[tid] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) {
        red_lo[tid] = red_lo[tid + h] < red_lo[tid] ? red_lo[tid + h] : red_lo[tid];
        red_hi[tid] = red_hi[tid + h] > red_hi[tid] ? red_hi[tid + h] : red_hi[tid];
      }
      __syncthreads();
    }
    lo = red_lo[0];
    const long long span = red_hi[0] - red_lo[0] + 1;
    in_lds = span <= kResampleWindow;
    if (in_lds) {
      for (int i = tid; i < (int)span; i += 256) win[i] = pcm_mono<T>(pcm, C, samples, ch_stride, s_stride, lo + i);
      __syncthreads();
    }
  }
  for (int r = tid; r < nout; r += 256) {
    float acc = 0.f;
    if (r < nlive) {
      const unsigned q = p0 + (unsigned)r, df = q / (unsigned)n, p = q - df * (unsigned)n;
      const long s = (f0 + df) * (long)o + first[p];
      const float* w = taps + p;
      if (in_lds) {
        const float* x = win + (int)(s - lo);
        for (int t = 0; t < K; ++t) acc = fmaf(w[(long)t * n], x[t], acc);
      } else {
        for (int t = 0; t < K; ++t) acc = fmaf(w[(long)t * n], pcm_mono<T>(pcm, C, samples, ch_stride, s_stride, s + t), acc);
      }
    }
    out[j0 + r] = acc;
  }
}

hipError_t launch_resample_mix(const void* pcm, bool s16, int channels, long samples, long ch_stride, long s_stride,
                               const float* taps, const int* first, int phases, int step, int K, float* out, long out_len,
                               long out_capacity, hipStream_t st) {
  if (out_capacity <= 0) return hipSuccess;
  // the most outputs whose window - (tile - 1) step / phases inputs plus, for a well-formed bank, at most 2 K + 4 - fits the LDS array
  const long fit = (long)(kResampleWindow - 2 * (long)K - 4) * phases / step + 1;
  const int tile = fit >= kResampleTileMax ? kResampleTileMax : (fit < 512 ? 256 : (int)(fit / 256) * 256);
  const long tiles = (out_capacity + tile - 1) / tile;
  if (tiles > 0x7fffffffL) return hipErrorInvalidValue;
  if (s16)
    hipLaunchKernelGGL(resample_mix_kernel<short>, dim3((unsigned)tiles), dim3(256), 0, st, (const short*)pcm, channels, samples,
                       ch_stride, s_stride, taps, first, phases, step, K, out, out_len, out_capacity, tile);
  else
    hipLaunchKernelGGL(resample_mix_kernel<float>, dim3((unsigned)tiles), dim3(256), 0, st, (const float*)pcm, channels, samples,
                       ch_stride, s_stride, taps, first, phases, step, K, out, out_len, out_capacity, tile);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Sound activity (samaudio.h samaudio_op_activity; the statement is tests/activity_ref.py): silence detection
// on `rows` mono waveforms and the overlap of the nonsilent spans with reference spans.  Everything behind the quantisation to
// int16 is integer arithmetic, so no result depends on the launch geometry, on `rows` or on the other rows.
//   activity_cells_kernel   waveform -> int16 -> 24 kHz by the closed form of audioop.ratecv -> cells[row][c] = sum of y^2 over the 24
//                           frames of millisecond c.  A workgroup owns kActivityTileCells consecutive cells; consecutive lanes take
//                           consecutive frames, so every input sample is fetched from memory once, in whole cache lines.
//   activity_score_kernel   one workgroup per row: cells -> sums per 10 ms in LDS (a window sum is 25 of them), the peak rms by an LDS
//                           max reduction, the silent flags of the window starts against the host's threshold table, then one thread
//                           walks pydub's detect_silence / detect_nonsilent and the reference's
//                           compute_iou_recall_precision in float64 with contraction off.
// ------------------------------------------------------------------------------------------------
constexpr int kActivityCellFrames = 24;       // frames per millisecond at 24 kHz
constexpr int kActivityWindowMs = 250;        // min_sil_ms and the peak window
constexpr int kActivitySeekMs = 10;           // seek_step
constexpr int kActivityPeakHopMs = 100;       // get_peak_rms's hop
constexpr int kActivityTileCells = 64;        // cells per workgroup of activity_cells_kernel: 1 536 frames, 6 per thread
constexpr int kActivityTileFrames = kActivityTileCells * kActivityCellFrames;
constexpr int kActivityDeca = kActivityWindowMs / kActivitySeekMs;   // decacells (10 ms) per window
constexpr int kActivityStartChunk = 2000;     // regular window starts whose decacells and flags are in LDS at a time (a multiple of 10 and of 8)

// clip(rint(x 32768), -32768, 32767), NaN -> 0.  The product with 2^15 is exact in fp32 (or overflows to an infinity, which the clip
// takes), so this is the statement's float64 expression.
__device__ __forceinline__ int activity_quantise(float x) {
  float v = x * 32768.f;
  if (!(v == v)) return 0;
  v = rintf(v);
  v = v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v);
  return (int)v;
}

__global__ __launch_bounds__(256) void activity_cells_kernel(const float* __restrict__ wav, long row_stride, int step, int phases,
                                                             long N, long L, long tiles, long long* __restrict__ cells) {
  __shared__ unsigned sq[kActivityTileFrames];
  const int tid = threadIdx.x;
  const long row = (long)blockIdx.x / tiles, tile = (long)blockIdx.x - row * tiles;
  const float* x = wav + row * row_stride;
  // frame j reads inputs m - 1 and m, m = ceil(step j / phases), with weights d = phases m - step j and phases - d.  step j is kept
  // as qf phases + rf and advanced by 256 frames at a time: one division per thread.
  const long inc = 256L * step, inc_q = inc / phases, inc_r = inc - inc_q * phases;
  long j = tile * kActivityTileFrames + tid;
  long qf = (long)step * j / phases, rf = (long)step * j - qf * phases;
  for (int r = tid; r < kActivityTileFrames; r += 256, j += 256) {
    unsigned v = 0;
    if (j < N) {   // m <= samples - 1 for every j < N = floor(phases (samples - 1) / step) + 1
      const long m = qf + (rf > 0 ? 1 : 0);
      const int d = rf > 0 ? (int)(phases - rf) : 0;
      const int a = d > 0 ? activity_quantise(x[m - 1]) : 0;   // (d > 0 implies m >= 1; x[-1] = 0 carries the weight 0 anyway)
      const int b = activity_quantise(x[m]);
      // trunc(65536 w / phases) >> 16 = floor(w / phases) for phases <= 65536: with w = q phases + t (truncated), the part below 2^16
      // is trunc(65536 t / phases), which is zero only for t = 0 and has the sign of w.  |w| <= 32768 phases < 2^31.
      const int w = a * d + b * (phases - d);
      int y = w / phases;
      if (w - y * phases < 0) --y;
      v = (unsigned)(y * y);
    }
    sq[r] = v;
    qf += inc_q;
    rf += inc_r;
    if (rf >= phases) {
      rf -= phases;
      ++qf;
    }
  }
  __syncthreads();
  if (tid < kActivityTileCells) {
    const long c = tile * kActivityTileCells + tid;
    if (c < L) {
      long long s = 0;
      for (int k = 0; k < kActivityCellFrames; ++k) s += sq[tid * kActivityCellFrames + k];
      cells[row * L + c] = s;
    }
  }
}

__device__ __forceinline__ int activity_isqrt(long long v) {
  long long r = (long long)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return (int)r;
}

// what the one walking thread carries: pydub's detect_silence / detect_nonsilent state and the sums of compute_iou_recall_precision
struct ActivityWalk {
  const double* ref;
  int n_ref;
  int* spans;
  int max_spans;
  int count = 0;            // nonsilent spans so far
  int silent_ranges = 0;
  bool have = false;        // a silent range is open
  long current = 0, prev = 0, prev_end = 0, last_end = 0;
  double total_hyp = 0.0, inter = 0.0;

  __device__ void emit(long a, long b) {   // one nonsilent span [a, b] ms
#pragma clang fp contract(off)
    if (spans && count < max_spans) {
      spans[2 * count] = (int)a;
      spans[2 * count + 1] = (int)b;
    }
    ++count;
    const double h0 = (double)a / 1000.0, h1 = (double)b / 1000.0;   // = round(a / 1000, 3) for an integer a
    total_hyp = total_hyp + (h1 - h0);
    for (int r = 0; r < n_ref; ++r) {
      const double r0 = ref[2 * r], r1 = ref[2 * r + 1];
      const double lo = r0 > h0 ? r0 : h0, hi = r1 < h1 ? r1 : h1, v = hi - lo;
      inter = inter + (v > 0.0 ? v : 0.0);
    }
  }
  __device__ void close(long a, long b) {   // one silent range [a, b]: the nonsilent span in front of it, unless that is a leading [0, 0]
    if (!(silent_ranges == 0 && a == 0)) emit(prev_end, a);
    prev_end = b;
    last_end = b;
    ++silent_ranges;
  }
  __device__ void silent_start(long pos) {
    if (!have) {
      have = true;
      current = pos;
    } else if (pos != prev + kActivitySeekMs && pos > prev + kActivityWindowMs) {
      close(current, prev + kActivityWindowMs);
      current = pos;
    }
    prev = pos;
  }
  __device__ void finish(long L) {
    if (!have) {
      emit(0, L);
      return;
    }
    close(current, prev + kActivityWindowMs);
    if (last_end != L) emit(prev_end, L);
  }
  __device__ float score(int metric) const {
#pragma clang fp contract(off)
    double total_ref = 0.0, sum = total_hyp;   // the union's sum runs over the hypothesis spans, then the reference spans
    for (int r = 0; r < n_ref; ++r) {
      const double len = ref[2 * r + 1] - ref[2 * r];
      total_ref = total_ref + len;
      sum = sum + len;
    }
    const double uni = sum - inter;
    const double den = metric == 0 ? uni : (metric == 1 ? total_ref : total_hyp);
    return n_ref > 0 && den > 0.0 ? (float)(inter / den) : 0.f;
  }
};

// the window starts range(0, last + 1, 10) are "regular": start 10 s sums the 25 decacells D[s .. s + 24], D[k] = cells[10 k .. 10 k + 9].
// They pass through LDS kActivityStartChunk at a time, once for the peak and once for the flags (a clip of up to 20.2 s is one chunk
// and is loaded once).  The start `last` itself, when it is no multiple of 10, sums its 250 cells on its own.
__global__ __launch_bounds__(256) void activity_score_kernel(const long long* __restrict__ cells, long L, const int* __restrict__ table,
                                                             const double* __restrict__ ref, int n_ref, int metric,
                                                             float* __restrict__ scores, int* __restrict__ spans, int max_spans,
                                                             int* __restrict__ span_count, int* __restrict__ peak_out) {
  __shared__ long long deca[kActivityStartChunk + kActivityDeca - 1];
  __shared__ long long part[256];
  __shared__ int red[256];
  __shared__ unsigned long long flagw[kActivityStartChunk / 8];
  constexpr int kWindowFrames = kActivityWindowMs * kActivityCellFrames;
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const long long* P = cells + row * L;
  ActivityWalk walk;
  walk.ref = ref;
  walk.n_ref = ref ? n_ref : 0;
  walk.spans = spans ? spans + row * 2L * max_spans : nullptr;
  walk.max_spans = max_spans;
  int peak = 0;
  if (L < kActivityWindowMs) {   // (uniform) shorter than one window: all of it is nonsilent
    if (tid == 0) walk.emit(0, L);
  } else {
    const long last = L - kActivityWindowMs;
    const long regular = last / kActivitySeekMs + 1;
    const bool odd_last = last % kActivitySeekMs != 0;
    // the decacells of the regular starts [s0, s0 + n): D[s0 .. s0 + n + 24); the last cell read is 10 (last / 10) + 249 <= L - 1
    auto load = [&](long s0, int n) {
      for (int k = tid; k < n + kActivityDeca - 1; k += 256) {
        const long long* c = P + (s0 + k) * kActivitySeekMs;
        long long d = 0;
        for (int e = 0; e < kActivitySeekMs; ++e) d += c[e];
        deca[k] = d;
      }
      __syncthreads();
    };
    auto window = [&](int s) {   // S(10 (s0 + s)): the sum of y^2 over the 6 000 frames of that window
      long long S = 0;
      for (int e = 0; e < kActivityDeca; ++e) S += deca[s + e];
      return S;
    };
    long loaded = -1;
    int mx = 0;
    for (long s0 = 0; s0 < regular; s0 += kActivityStartChunk) {
      const int n = regular - s0 < kActivityStartChunk ? (int)(regular - s0) : kActivityStartChunk;
      if (loaded >= 0) __syncthreads();   // (every thread is done with the chunk before)
      load(s0, n);
      loaded = s0;
      const int hop = kActivityPeakHopMs / kActivitySeekMs;
      for (int s = tid * hop; s < n; s += 256 * hop) {   // (kActivityStartChunk is a multiple of hop: s0 + s is one too)
        const int rms = activity_isqrt(window(s) / kWindowFrames);
        mx = rms > mx ? rms : mx;
      }
    }
    red[tid] = mx;
    // the window that starts at `last`, where the regular starts do not reach it
    part[tid] = odd_last && tid < kActivityWindowMs ? P[last + tid] : 0;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) {
        red[tid] = red[tid + h] > red[tid] ? red[tid + h] : red[tid];
        part[tid] += part[tid + h];
      }
      __syncthreads();
    }
    peak = red[0] > 32768 ? 32768 : red[0];
    int T = table[peak];
    T = T < 0 ? 0 : (T > 65535 ? 65535 : T);
    const long long limit = (long long)(T + 1) * (T + 1) * kWindowFrames;   // rms <= thresh <=> S < limit
    const bool last_silent = odd_last && part[0] < limit;
    unsigned char* flags = (unsigned char*)flagw;
    for (long s0 = 0; s0 < regular; s0 += kActivityStartChunk) {
      const int n = regular - s0 < kActivityStartChunk ? (int)(regular - s0) : kActivityStartChunk;
      if (loaded != s0) {
        __syncthreads();
        load(s0, n);
        loaded = s0;
      }
      for (int s = tid; s < n; s += 256) flags[s] = window(s) < limit ? 1 : 0;
      __syncthreads();
      if (tid == 0) {
        // eight starts at a time: a word of ones is one run (its first start may open or close a range, the others follow at + 10)
        for (int s = 0; s < n; s += 8) {
          const unsigned long long w = flagw[s >> 3];
          const long pos = (s0 + s) * kActivitySeekMs;
          if (s + 8 <= n && w == 0x0101010101010101ULL) {
            walk.silent_start(pos);
            walk.prev = pos + 7 * kActivitySeekMs;
          } else if (s + 8 > n || w != 0) {
            for (int e = 0; e < 8 && s + e < n; ++e)
              if ((w >> (8 * e)) & 0xff) walk.silent_start(pos + e * kActivitySeekMs);
          }
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (last_silent) walk.silent_start(last);
      walk.finish(L);
    }
  }
  if (tid == 0) {
    scores[row] = walk.score(metric);
    if (span_count) span_count[row] = walk.count;
    if (peak_out) peak_out[row] = peak;
  }
}

hipError_t launch_activity(const float* wav, int rows, long row_stride, int step, int phases, long N, long L, const int* table,
                           const double* ref_spans, int n_ref, int metric, long long* cells, float* scores, int* spans,
                           int max_spans, int* span_count, int* peak, hipStream_t st) {
  const long tiles = (L + kActivityTileCells - 1) / kActivityTileCells;
  if (tiles * rows > 0x7fffffffL) return hipErrorInvalidValue;
  if (tiles > 0)
    hipLaunchKernelGGL(activity_cells_kernel, dim3((unsigned)(tiles * rows)), dim3(256), 0, st, wav, row_stride, step, phases, N, L,
                       tiles, cells);
  hipLaunchKernelGGL(activity_score_kernel, dim3((unsigned)rows), dim3(256), 0, st, cells, L, table, ref_spans, n_ref, metric, scores,
                     spans, max_spans, span_count, peak);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// CLAP log-mel front end (samaudio.h samaudio_op_logmel; the statement is tests/clap_ref.py): waveform rows ->
// [frames, n_mels] dB features in one kernel.  A workgroup owns `fb` consecutive frames of one row (fb M <= kLogmelPoints complex
// points, M = N / 2) and keeps everything between the waveform and the features in LDS:
//   load      sample 2t | 2t + 1 of a frame -> the int16 round trip, repeatpad / crop and the reflection as index arithmetic on the
//             load, times the window -> z[bitrev(t)] = (even, odd): the real frame packed as M complex points
//   fft       log2 M radix-2 decimation-in-time passes in place, twiddles from the caller's float64-evaluated table
//   untangle  X[k] = E[k] + w^k O[k], E / O from Z[k] and conj Z[M - k], k <= M; P[k] = |X[k]|^2.  A frame of zeros gives exact zeros
//             (no frame shares a transform with another one)
//   mel       16 features per wave at a time, each summed by 4 lanes over k = j, j + 4, ... and folded by two xor shuffles (a fixed
//             order: the result does not depend on the launch geometry); 10 log10, the floor, the per-mel scale and shift
// ------------------------------------------------------------------------------------------------
constexpr int kLogmelPoints = 2048;      // complex points of z: fb = min(kLogmelMaxFrames, kLogmelPoints / M) frames per workgroup
constexpr int kLogmelMaxFrames = 8;
constexpr float kClapInt16Scale = 32767.0f;   // samaudio.h SAMAUDIO_CLAP_INT16_SCALE

// laion_clap's int16_to_float32_torch(float32_to_int16_torch(x)): clamp, x 32767 rounded to fp32, truncated toward zero, / 32767
// rounded to fp32 (nothing can be contracted into the product: the truncation stands between it and the division)
__device__ __forceinline__ float clap_quantise(float x) {
  x = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);
  return truncf(x * kClapInt16Scale) / kClapInt16Scale;
}

// sample p of the padded clip, p in [-N / 2, L + N / 2): reflected into [0, L) (N / 2 < L), then the crop x[offset + p] of a longer
// clip, or x[p % n] below rep_end = (L / n) n and zero behind
__device__ __forceinline__ float clap_sample(const float* __restrict__ x, unsigned n, long offset, int L, unsigned rep_end, bool longer,
                                             bool quantise, int p) {
  if (p < 0) p = -p;
  if (p >= L) p = 2 * (L - 1) - p;
  float v;
  if (longer) v = x[offset + p];
  else if ((unsigned)p < rep_end) v = x[(unsigned)p % n];
  else return 0.f;
  return quantise ? clap_quantise(v) : v;
}

__global__ __launch_bounds__(256) void clap_logmel_kernel(const float* __restrict__ wav, long row_stride, unsigned n, long offset, int L,
                                                          unsigned rep_end, int longer, int quantise, int log2n, int hop, int n_mels,
                                                          int frames, int fb, const float* __restrict__ tables,
                                                          const float* __restrict__ bank, const float* __restrict__ bn_scale,
                                                          const float* __restrict__ bn_shift, float* __restrict__ out) {
  __shared__ float2 z[kLogmelPoints];
  __shared__ float2 tw[kLogmelPoints / 2];
  __shared__ float win[kLogmelPoints];
  __shared__ float pw[kLogmelPoints + kLogmelMaxFrames];
  const int tid = threadIdx.x, N = 1 << log2n, M = N >> 1, logm = log2n - 1, nb = M + 1;
  const int row = blockIdx.y, f0 = (int)blockIdx.x * fb, nf = frames - f0 < fb ? frames - f0 : fb;
  const float* x = wav + (long)row * row_stride;
  for (int i = tid; i < N; i += 256) win[i] = tables[i];
  for (int i = tid; i < M; i += 256) tw[i] = make_float2(tables[N + 2 * i], tables[N + 2 * i + 1]);
  __syncthreads();
  for (int i = tid; i < nf * M; i += 256) {
    const int f = i >> logm, t = i & (M - 1), p = (f0 + f) * hop - M + 2 * t;
    const float a = clap_sample(x, n, offset, L, rep_end, longer != 0, quantise != 0, p) * win[2 * t];
    const float b = clap_sample(x, n, offset, L, rep_end, longer != 0, quantise != 0, p + 1) * win[2 * t + 1];
    z[(f << logm) + (int)(__builtin_bitreverse32((unsigned)t) >> (32 - logm))] = make_float2(a, b);
  }
  __syncthreads();
  for (int s = 0; s < logm; ++s) {
    const int half = 1 << s;
    for (int i = tid; i < nf * (M >> 1); i += 256) {
      const int f = i >> (logm - 1), b = i & ((M >> 1) - 1), pos = b & (half - 1);
      const int i0 = (f << logm) + ((b >> s) << (s + 1)) + pos, i1 = i0 + half;
      const float2 w = tw[pos << (logm - s)];   // exp(-2 pi i pos / (2 half)) = entry pos N / (2 half) of the table over N
      const float2 u = z[i0], v = z[i1];
      const float tr = v.x * w.x - v.y * w.y, ti = v.x * w.y + v.y * w.x;
      z[i0] = make_float2(u.x + tr, u.y + ti);
      z[i1] = make_float2(u.x - tr, u.y - ti);
    }
    __syncthreads();
  }
  for (int i = tid; i < nf * nb; i += 256) {
    const int f = i / nb, k = i - f * nb;
    const float2 a = z[(f << logm) + (k & (M - 1))], b = z[(f << logm) + ((M - k) & (M - 1))];
    const float er = 0.5f * (a.x + b.x), ei = 0.5f * (a.y - b.y);     // E = (Z[k] + conj Z[M - k]) / 2
    const float qr = 0.5f * (a.y + b.y), qi = -0.5f * (a.x - b.x);    // O = (Z[k] - conj Z[M - k]) / 2i
    const float2 w = k < M ? tw[k] : make_float2(-1.f, 0.f);
    const float xr = er + (qr * w.x - qi * w.y), xi = ei + (qr * w.y + qi * w.x);
    pw[i] = xr * xr + xi * xi;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, j = lane >> 4, total = nf * n_mels;
  for (int base = 0; base < total; base += 64) {
    const int o = base + wave * 16 + (lane & 15);
    int f = 0, m = 0;
    float s = 0.f;
    if (o < total) {
      f = o / n_mels;
      m = o - f * n_mels;
      const float* pf = pw + f * nb;
      for (int k = j; k < nb; k += 4) s = fmaf(bank[(long)k * n_mels + m], pf[k], s);
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (o < total && j == 0) {
      float d = s > 1e-10f ? 10.f * log10f(s) : -100.f;
      if (bn_scale) d = d * bn_scale[m] + bn_shift[m];
      out[((long)row * frames + f0 + f) * n_mels + m] = d;
    }
  }
}

hipError_t launch_clap_logmel(const float* wav, int rows, long row_stride, long n, long offset, int L, bool quantise, int log2n, int hop,
                              int n_mels, int frames, const float* tables, const float* bank, const float* bn_scale,
                              const float* bn_shift, float* out, hipStream_t st) {
  const int M = 1 << (log2n - 1);
  if (log2n < 6 || M > kLogmelPoints / 2 || rows < 1 || rows > 65535 || n < 1 || frames < 1) return hipErrorInvalidValue;
  const int fb = kLogmelPoints / M < kLogmelMaxFrames ? kLogmelPoints / M : kLogmelMaxFrames;
  const bool longer = n > L;
  const unsigned nn = longer ? 0u : (unsigned)n, rep_end = longer ? 0u : (unsigned)((L / n) * n);
  hipLaunchKernelGGL(clap_logmel_kernel, dim3((unsigned)((frames + fb - 1) / fb), (unsigned)rows), dim3(256), 0, st, wav, row_stride, nn,
                     longer ? offset : 0L, L, rep_end, longer ? 1 : 0, quantise ? 1 : 0, log2n, hop, n_mels, frames, fb, tables, bank,
                     bn_scale, bn_shift, out);
  return hipGetLastError();
}

// SAMAUDIO_OPT_SENTINEL (engine.hip): largest magnitude and number of non-finite values of a 16-bit (or fp32) tensor [rows, cols]
// with row pitch ld, folded into a per-class slot {float absmax, float nonfinite count} - two launches on the launch stream, no
// atomics (partials per workgroup, then one workgroup folds them into the slot; launches of a stream are ordered).  A debugging /
// validation aid: an fp16 operand that overflowed is REPORTED with its class, not propagated silently.
template <typename T> struct SentinelLoad;
template <> struct SentinelLoad<float> { static __device__ float ld(const float* p) { return *p; } };
template <> struct SentinelLoad<bf16_t> { static __device__ float ld(const bf16_t* p) { return bf2f(p->v); } };
template <> struct SentinelLoad<alt16_t> { static __device__ float ld(const alt16_t* p) { return __uint_as_float(((unsigned)p->v) << 16); } };
template <typename T>
__global__ __launch_bounds__(256) void sentinel_scan_kernel(const T* __restrict__ x, long rows, int cols, long ld, float* __restrict__ partial) {
  float mx = 0.f, bad = 0.f;
  const long total = rows * cols;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const float v = SentinelLoad<T>::ld(x + (i / cols) * ld + (i % cols));
    // NaN and +-Inf only (exponent bits all set): the finite values above 3.0e38 - bfloat16's 0x7f62 .. 0x7f7f, fp32's top - are
    // magnitudes, as samaudio.h says "non-finite" (before, `fabsf(v) > 3.0e38f` counted them as non-finite)
    if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) bad += 1.f;
    else mx = fmaxf(mx, fabsf(v));
  }
  __shared__ float smx[256], sbad[256];
  smx[threadIdx.x] = mx;
  sbad[threadIdx.x] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
      sbad[threadIdx.x] += sbad[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = smx[0];
    partial[2 * blockIdx.x + 1] = sbad[0];
  }
}
__global__ void sentinel_fold_kernel(const float* __restrict__ partial, int n, float* __restrict__ slot) {
  if (threadIdx.x != 0) return;
  float mx = slot[0], bad = slot[1];
  for (int i = 0; i < n; ++i) {
    mx = fmaxf(mx, partial[2 * i]);
    bad += partial[2 * i + 1];
  }
  slot[0] = mx;
  slot[1] = bad;
}
// fmt: 0 = fp32, 1 = the library's 16-bit operand format, 2 = the alt 16-bit format (bfloat16)
hipError_t launch_sentinel(const void* x, int fmt, long rows, int cols, long ld, float* partial, float* slot, hipStream_t st) {
  if (!x || rows <= 0 || cols <= 0) return hipSuccess;
  const long total = rows * cols;
  int grid = (int)((total + 256 * 16 - 1) / (256 * 16));
  grid = grid < 1 ? 1 : (grid > kSentinelPartials ? kSentinelPartials : grid);
  if (fmt == 0) hipLaunchKernelGGL(sentinel_scan_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x, rows, cols, ld, partial);
  else if (fmt == 1) hipLaunchKernelGGL(sentinel_scan_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, rows, cols, ld, partial);
  else hipLaunchKernelGGL(sentinel_scan_kernel<alt16_t>, dim3(grid), dim3(256), 0, st, (const alt16_t*)x, rows, cols, ld, partial);
  hipLaunchKernelGGL(sentinel_fold_kernel, dim3(1), dim3(64), 0, st, partial, grid, slot);
  return hipGetLastError();
}

// SAMAUDIO_TRACE_HASH (engine.hip): one 64-bit checksum per batch item of a stage's buffer, on the launch stream
__global__ __launch_bounds__(256) void hash_items_kernel(const unsigned* x, size_t words, unsigned long long* out) {
  const unsigned* src = x + (size_t)blockIdx.x * words;
  unsigned long long h = 0;
  for (size_t i = threadIdx.x; i < words; i += 256) h += (unsigned long long)(src[i] ^ (unsigned)(i * 0x9E3779B1u)) * (2 * i + 1);
  __shared__ unsigned long long part[256];
  part[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}
hipError_t launch_hash_items(const unsigned* x, size_t words_per_item, int items, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(hash_items_kernel, dim3(items), dim3(256), 0, st, x, words_per_item, out);
  return hipGetLastError();
}
bool sentinel_built() { return true; }
void* debug_device_alloc(size_t bytes) {   // debugging aids only: the product path never allocates device memory
  void* p = nullptr;
  return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
void debug_device_free(void* p) { if (p) (void)hipFree(p); }

}  // namespace sa
