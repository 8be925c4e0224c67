// The laser-scan expansion of the DFormerTrav backbone (models/encoders/DFormer.py:308-339
// Attention1Dto2D, called at DFormer.py:444) collapsed to what it computes. attn2
// attends over one key, so its softmax is 1 and the returned plane [B, 1, Hout, L] is constant along
// Hout; input_proj is Linear(1, E), so attn1's scores are affine in the scalar range x[b][j]. With
// alpha [L][Hh], g [Hh] and c folded from the parameters (encoder.Attention1Dto2D.fold):
//   mean[b][l][h] = sum_j softmax_j(alpha[l][h] * x[b][j]) * x[b][j]
//   var[b][l][h]  = sum_j softmax_j(alpha[l][h] * x[b][j]) * (x[b][j] - mean[b][l][h])^2
//   s[b][l]       = c + sum_h g[h] * mean[b][l][h],     plane[b][y][l] = s[b][l] for every y < Hout
//   dfm_laser_expand_fwd  x, alpha, g, c -> s, plane [, mean, var]
//   dfm_laser_expand_bwd  dplane, g, mean, var -> ds, dalpha, dg, dc
// A workgroup stages one image's scan in LDS, shifted by the scan's mean (the moments are taken about
// it, as the BN statistics of this library are). kJ neighbouring lanes share one (l, h) pair: lane jl
// walks the ranges jl, jl + kJ, ... as LDS reads (a wave reads kJ consecutive words, each broadcast)
// and the kJ partial moments combine by lane shuffles; one lane per pair would leave 640 waves at
// bs 16, fewer than the chip has SIMDs, each walking all N ranges. The softmax's maximum is analytic:
// alpha * max_j x or alpha * min_j x by the sign of alpha, so the weights are
// exp(alpha * (x_j - x_ref)) <= 1 with one of them exactly 1 and no running rescale is needed. The
// variance is a second walk about the pair's own mean (E[x^2] - mean^2 cancels when the softmax is
// sharp); it is skipped when var is NULL (inference). The heads of a column sit kJ lanes apart: they
// combine by lane shuffles and the column segment is written down the rows.
// Every sum runs in a fixed order (strided per-thread sums, xor butterflies, partials combined in
// ascending order): no float atomics, so two runs agree bit for bit. The scan is input data: no
// gradient with respect to it is computed.
#include <math.h>

#include "common.h"

namespace {

constexpr int kFwdThreads = 512;  // cols columns x Hp head lanes x kJ range lanes (Hp: Hh rounded up to 2^k)
constexpr int kFwdWaves = kFwdThreads / 64;
constexpr int kJ = 4;
constexpr int kMaxHeads = 8;
constexpr int kDsCols = 64, kDsRows = 8;  // dfm_laser_expand_bwd's row sum: 64 columns x 8 row chunks
constexpr int kGradThreads = 256;
constexpr int kGradVals = kMaxHeads + 1;  // a workgroup's partial dg[0 .. 8) and dc

DFM_INLINE float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(kFwdThreads) void laser_expand_fwd_kernel(
    int N, int L, int Hh, int Hp, int Hout, const float* __restrict__ x, const float* __restrict__ alpha,
    const float* __restrict__ g, const float* __restrict__ c, float* __restrict__ s, float* __restrict__ mean,
    float* __restrict__ var, float* __restrict__ plane) {
  extern __shared__ float sm[];  // xs[N] (the shifted scan), red[3][kFwdWaves], sb[cols]
  float* xs = sm;
  float* red = sm + N;
  float* sb = red + 3 * kFwdWaves;
  const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.y;
  const int cols = kFwdThreads / (Hp * kJ);
  const float* xb = x + (long)b * N;

  float part = 0.f;
  for (int j = tid; j < N; j += kFwdThreads) part += xb[j];
  part = wave_sum(part);
  if ((tid & 63) == 0) red[wave] = part;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < kFwdWaves; ++w) tot += red[w];
  const float shift = tot / (float)N;
  float lo = INFINITY, hi = -INFINITY;
  for (int j = tid; j < N; j += kFwdThreads) {
    const float v = xb[j] - shift;
    xs[j] = v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((tid & 63) == 0) {
    red[kFwdWaves + wave] = lo;
    red[2 * kFwdWaves + wave] = hi;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kFwdWaves; ++w) {
    lo = fminf(lo, red[kFwdWaves + w]);
    hi = fmaxf(hi, red[2 * kFwdWaves + w]);
  }

  const int jl = tid % kJ, h = (tid / kJ) % Hp, col = tid / (kJ * Hp);
  const int l = blockIdx.x * cols + col;
  const bool active = l < L && h < Hh;
  const float a = active ? alpha[(long)l * Hh + h] : 0.f;
  const float ref = a >= 0.f ? hi : lo;  // alpha * (x_j - ref) <= 0, and 0 at the maximum
  float z = 0.f, s1 = 0.f;
  for (int j = jl; j < N; j += kJ) {
    const float t = xs[j];
    const float w = __expf(a * (t - ref));
    z += w;
    s1 = fmaf(w, t, s1);
  }
  z = group_sum<kJ>(z);  // the butterfly leaves the same bits in the kJ lanes of a pair
  s1 = group_sum<kJ>(s1);
  const float inv = 1.f / z;  // z >= 1: the maximum's weight is 1
  const float m = s1 * inv;   // the weighted mean, about the shift
  const float mu = shift + m;
  if (var != nullptr) {
    float s2 = 0.f;
    for (int j = jl; j < N; j += kJ) {
      const float t = xs[j];
      const float w = __expf(a * (t - ref));
      const float d = t - m;
      s2 = fmaf(w, d * d, s2);
    }
    s2 = group_sum<kJ>(s2);
    if (active && jl == 0) {
      const long i = ((long)b * L + l) * Hh + h;
      mean[i] = mu;
      var[i] = s2 * inv;
    }
  }
  float acc = active ? g[h] * mu : 0.f;
  for (int o = (Hp >> 1) * kJ; o >= kJ; o >>= 1) acc += __shfl_xor(acc, o, 64);
  acc += c[0];
  if (h == 0 && jl == 0) {
    sb[col] = acc;
    if (l < L) s[(long)b * L + l] = acc;
  }
  __syncthreads();
  // thread (row tid / cols, column tid % cols) of the cols-wide segment: consecutive lanes write
  // consecutive floats of a plane row
  const int cc = tid % cols, lw = blockIdx.x * cols + cc;
  if (lw < L) {
    const float v = sb[cc];
    float* dst = plane + (long)b * Hout * L + lw;
    for (int y = tid / cols; y < Hout; y += kFwdThreads / cols) dst[(long)y * L] = v;
  }
}

// ds[b][l] = sum_y dplane[b][y][l]: kDsRows lanes share a column, each sums its contiguous chunk of
// rows in ascending y, and the chunks are combined in ascending order.
__global__ __launch_bounds__(kDsCols * kDsRows) void laser_rowsum_kernel(int L, int Hout,
                                                                          const float* __restrict__ dplane,
                                                                          float* __restrict__ ds) {
  __shared__ float part[kDsRows][kDsCols];
  const int cl = threadIdx.x % kDsCols, r = threadIdx.x / kDsCols, b = blockIdx.y;
  const int l = blockIdx.x * kDsCols + cl;
  const int chunk = (Hout + kDsRows - 1) / kDsRows;
  const int y0 = r * chunk, y1 = min(y0 + chunk, Hout);
  float acc = 0.f;
  if (l < L) {
    const float* src = dplane + (long)b * Hout * L + l;
#pragma unroll 8
    for (int y = y0; y < y1; ++y) acc += src[(long)y * L];
  }
  part[r][cl] = acc;
  __syncthreads();
  if (r == 0 && l < L) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kDsRows; ++i) v += part[i][cl];
    ds[(long)b * L + l] = v;
  }
}

// One thread per (l, h), i = l * Hh + h, sums over the batch in ascending b:
//   dalpha[i] = g[h] * sum_b ds[b][l] * var[b][l][h];   pm = sum_b ds[b][l] * mean[b][l][h];   pc = sum_b ds[b][l]
// and the workgroup leaves partials[blockIdx][h] = the sum of its pm of head h in ascending i, and
// partials[blockIdx][8] = the sum of its pc over its columns (the h == 0 threads) in ascending i.
__global__ __launch_bounds__(kGradThreads) void laser_param_grad_kernel(
    int B, int L, int Hh, const float* __restrict__ ds, const float* __restrict__ g, const float* __restrict__ mean,
    const float* __restrict__ var, float* __restrict__ dalpha, float* __restrict__ partials) {
  __shared__ float pm_s[kGradThreads], pc_s[kGradThreads];
  const int tid = threadIdx.x;
  const long i0 = (long)blockIdx.x * kGradThreads, i = i0 + tid;
  float av = 0.f, pm = 0.f, pc = 0.f;
  if (i < (long)L * Hh) {
    const int l = (int)(i / Hh), h = (int)(i % Hh);
    for (int b = 0; b < B; ++b) {
      const float d = ds[(long)b * L + l];
      const long k = ((long)b * L + l) * Hh + h;
      av = fmaf(d, var[k], av);
      pm = fmaf(d, mean[k], pm);
      pc += d;
    }
    dalpha[i] = g[h] * av;
  }
  pm_s[tid] = pm;
  pc_s[tid] = pc;
  __syncthreads();
  if (tid < Hh || tid == kMaxHeads) {
    const int h = tid == kMaxHeads ? 0 : tid;
    const float* src = tid == kMaxHeads ? pc_s : pm_s;
    float v = 0.f;
    int k = (int)((h - i0 % Hh + Hh) % Hh);  // the first thread of head h in this workgroup
    for (; k < kGradThreads; k += Hh) v += src[k];  // threads past L * Hh hold zeros
    partials[(long)blockIdx.x * kGradVals + tid] = v;
  }
}

// dg[h] = sum over the workgroups' partials in ascending order, likewise dc.
__global__ __launch_bounds__(64) void laser_param_grad_final_kernel(int nblk, int Hh,
                                                                     const float* __restrict__ partials,
                                                                     float* __restrict__ dg, float* __restrict__ dc) {
  const int tid = threadIdx.x;
  if (tid < Hh || tid == kMaxHeads) {
    float v = 0.f;
    for (int k = 0; k < nblk; ++k) v += partials[(long)k * kGradVals + tid];
    if (tid == kMaxHeads) dc[0] = v;
    else dg[tid] = v;
  }
}

}  // namespace

extern "C" int dfm_laser_expand_fwd(int B, int N, int L, int Hh, int Hout, const float* x, const float* alpha,
                                    const float* g, const float* c, float* s, float* mean, float* var, float* plane,
                                    dfm_stream_t stream) {
  DFM_CHECK_ARG(x && alpha && g && c && s && plane, "dfm_laser_expand_fwd: null pointer");
  DFM_CHECK_ARG((mean != nullptr) == (var != nullptr), "dfm_laser_expand_fwd: mean and var go together");
  DFM_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && L > 0 && Hout > 0,
                "dfm_laser_expand_fwd: bad argument (B=%d in [1, 65535], N=%d, L=%d, Hout=%d must be positive)", B, N,
                L, Hout);
  DFM_CHECK_ARG(N <= DFM_LASER_MAX_N, "dfm_laser_expand_fwd: N=%d exceeds the %d ranges a workgroup stages in LDS", N,
                DFM_LASER_MAX_N);
  DFM_CHECK_ARG(Hh > 0 && Hh <= kMaxHeads, "dfm_laser_expand_fwd: Hh=%d outside [1, %d]", Hh, kMaxHeads);
  int Hp = 1;
  while (Hp < Hh) Hp <<= 1;
  const int cols = kFwdThreads / (Hp * kJ);
  const size_t lds = (size_t)(N + 3 * kFwdWaves + cols) * sizeof(float);
  DFM_LAUNCH(laser_expand_fwd_kernel, dim3(cdiv(L, cols), B), dim3(kFwdThreads), lds, (hipStream_t)stream, N, L, Hh, Hp,
             Hout, x, alpha, g, c, s, mean, var, plane);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" size_t dfm_laser_expand_bwd_workspace(int L, int Hh) {
  if (L <= 0 || Hh <= 0 || Hh > kMaxHeads) return 0;
  return (size_t)cdiv((long)L * Hh, kGradThreads) * kGradVals * sizeof(float);
}

extern "C" int dfm_laser_expand_bwd(int B, int L, int Hh, int Hout, const float* dplane, const float* g,
                                    const float* mean, const float* var, float* ds, float* dalpha, float* dg,
                                    float* dc, void* workspace, dfm_stream_t stream) {
  DFM_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && Hout > 0,
                "dfm_laser_expand_bwd: bad argument (B=%d in [1, 65535], L=%d, Hout=%d must be positive)", B, L, Hout);
  DFM_CHECK_ARG(Hh > 0 && Hh <= kMaxHeads, "dfm_laser_expand_bwd: Hh=%d outside [1, %d]", Hh, kMaxHeads);
  DFM_CHECK_ARG(dplane && g && mean && var && ds && dalpha && dg && dc && workspace,
                "dfm_laser_expand_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  float* partials = (float*)workspace;
  const int nblk = (int)cdiv((long)L * Hh, kGradThreads);
  DFM_LAUNCH(laser_rowsum_kernel, dim3(cdiv(L, kDsCols), B), dim3(kDsCols * kDsRows), 0, st, L, Hout, dplane, ds);
  DFM_LAUNCH_CHECK();
  DFM_LAUNCH(laser_param_grad_kernel, dim3(nblk), dim3(kGradThreads), 0, st, B, L, Hh, ds, g, mean, var, dalpha,
             partials);
  DFM_LAUNCH_CHECK();
  DFM_LAUNCH(laser_param_grad_final_kernel, dim3(1), dim3(64), 0, st, nblk, Hh, partials, dg, dc);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
