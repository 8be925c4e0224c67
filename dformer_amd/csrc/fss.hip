// The few-shot tail of EncoderDecoder.meta_forward (models/builder.py:237-320), collapsed onto stage-3
// sized tensors. Bilinear interpolation is linear, so the masked average pooling of the
// upsampled support features (get_masked_proto, builder.py:312-317) is a weighted sum of the h' x w'
// feature rows themselves, the weights being the adjoint of the upsample applied to the class mask (the
// mask "footprint"); nothing of size C x H x W is formed.
//   dfm_fss_mask_footprint   masks [n][H][W] int64 -> foot [n][2][h'][w'], count [n][2]   (279-280, 313-316)
//   dfm_fss_proto_pool_fwd   foot, count, support rows -> proto [B][2][C]                 (281-288, 315-316)
//   dfm_fss_sim_fwd / _bwd   query rows, proto -> prob [B*h'*w'][2]                       (294-297, 319-320)
//   dfm_fss_loss_fwd / _bwd  alpha up(L) + (1 - alpha) up(prob), CE, mean over != 255     (298-308)
//   dfm_fss_fuse_fwd         the fused full-resolution logits themselves (eval)           (298-303)
// The adjoint of the upsample of a one-channel plane is separable, A_y^T M A_x with two non-zeros per
// row of each A: an x-pass stages rows of the plane in LDS and every (row, low-res column) sums its
// pixels in ascending x; a y-pass sums, per low-res cell, 8 chunks of rows in ascending y and combines
// them in ascending order. The footprint (M = the class indicator) and both gradients of the loss (M =
// softmax_1 - onehot_1, one float per pixel: with two classes g_0 = -g_1) are this pair of kernels.
// The prototype pool and the cosine's backward are the same two shapes, a [2 x rows] . [rows x C]
// weighted row sum and a rank-2 outer product, and share rowsum2 / outer2 below.
// Every sum runs in a fixed order and there are no float atomics: two runs agree bit for bit.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

// the taps of F.interpolate(mode="bilinear", align_corners=False), as csrc/loss.hip has them
DFM_INLINE void src_idx(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}
// a conservative lower bound of the pixels whose taps reach low-res index j (taps are then tested exactly)
DFM_INLINE int first_pixel(int j, int in, int out) {
  const float inv = (float)out / (float)in;
  return max(0, (int)floorf(((float)j + 0.5f) * inv - 0.5f) - 2);
}
// and an upper bound (exclusive) of the pixels whose first tap is <= j
DFM_INLINE int end_pixel(int j, int in, int out) {
  const float inv = (float)out / (float)in;
  return min(out, (int)ceilf(((float)j + 1.5f) * inv - 0.5f) + 2);
}
// the weight of low-res index j in pixel x's pair of taps (clamped duplicates merge)
DFM_INLINE float tap_weight(int x, int j, int in, int out, bool& past) {
  int i0, i1;
  float l1;
  src_idx(x, in, out, i0, i1, l1);
  past = i0 > j;
  return (i0 == j ? 1.f - l1 : 0.f) + (i1 == j ? l1 : 0.f);
}

// ------------------------------------------------------------------ adjoint of the upsample, x-pass
constexpr int kXT = 256;
constexpr int kXRowsMax = 8;
constexpr int kXMaxFloats = 12288;  // LDS floats a workgroup stages (48 KB): R rows of W pixels

// MASK: src is int64 [n][H][W]; rx [n][2][H][w], rx[n][k][y][j] = sum_x wx(x, j) [src == k], and
//   cntpart[n][blk][k] = the workgroup's count of pixels == k (an exact integer in float32).
// else: src is float32 [n][H][W]; rx [n][H][w] = sum_x wx(x, j) src.
// The R rows of a workgroup are contiguous in memory and are read as 16-byte vectors.
template <bool MASK>
__global__ __launch_bounds__(kXT) void fss_adjoint_xpass_kernel(int H, int W, int w, int R,
                                                                const void* __restrict__ src_,
                                                                float* __restrict__ rx,
                                                                float* __restrict__ cntpart) {
  extern __shared__ __attribute__((aligned(16))) float row[];  // [R][W]
  __shared__ float cred[2][kXT / 64];
  const int tid = threadIdx.x, n = blockIdx.y, y0 = blockIdx.x * R, rows = min(R, H - y0);
  const long e0 = ((long)n * H + y0) * W;
  const int cnt = rows * W;
  if constexpr (MASK) {
    const long long* src = (const long long*)src_ + e0;
    float c0 = 0.f, c1 = 0.f;
    auto put = [&](int i, long long v) {
      row[i] = v == 0 ? 0.f : (v == 1 ? 1.f : -1.f);
      c0 += v == 0 ? 1.f : 0.f;
      c1 += v == 1 ? 1.f : 0.f;
    };
    const int head = min(cnt, (int)(((uintptr_t)src & 15) / 8));
    const int npair = (cnt - head) / 2;
    if (tid == 0 && head) put(0, src[0]);
    for (int q = tid; q < npair; q += kXT) {
      const longlong2 v = *reinterpret_cast<const longlong2*>(src + head + 2 * q);
      put(head + 2 * q, v.x);
      put(head + 2 * q + 1, v.y);
    }
    if (tid == 0 && head + 2 * npair < cnt) put(cnt - 1, src[cnt - 1]);
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    if ((tid & 63) == 0) {
      cred[0][tid >> 6] = c0;
      cred[1][tid >> 6] = c1;
    }
  } else {
    const float* src = (const float*)src_ + e0;
    const int mis = (int)((uintptr_t)src & 15);
    const int head = min(cnt, mis ? (16 - mis) / 4 : 0);
    const int nquad = (cnt - head) / 4;
    if (tid < head) row[tid] = src[tid];
    for (int q = tid; q < nquad; q += kXT) {
      const float4 v = *reinterpret_cast<const float4*>(src + head + 4 * q);
      float* d = row + head + 4 * q;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    const int done = head + 4 * nquad;
    if (tid < cnt - done) row[done + tid] = src[done + tid];
  }
  __syncthreads();
  if constexpr (MASK) {
    if (tid < 2) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < kXT / 64; ++q) v += cred[tid][q];
      cntpart[((long)n * gridDim.x + blockIdx.x) * 2 + tid] = v;
    }
  }
  constexpr int NK = MASK ? 2 : 1;
  for (int e = tid; e < rows * NK * w; e += kXT) {
    const int j = e % w, k = (e / w) % NK, r = e / (NK * w);
    const float* rr = row + r * W;
    float acc = 0.f;
    for (int x = first_pixel(j - 1, w, W); x < W; ++x) {
      bool past;
      const float wx = tap_weight(x, j, w, W, past);
      if (past) break;  // taps are monotone in x
      const float v = MASK ? (rr[x] == (float)k ? 1.f : 0.f) : rr[x];
      acc = fmaf(wx, v, acc);
    }
    rx[(((long)n * NK + k) * H + (y0 + r)) * w + j] = acc;
  }
}

// ------------------------------------------------------------------ adjoint of the upsample, y-pass
constexpr int kYCells = 32, kYChunks = 8;

// rx [P][H][w] -> per low-res cell (p, i, j): v = sum_y wy(y, i) rx[p][y][j].
// PAIR false: out [P][h][w] float32 = v (the footprint).
// PAIR true:  out [P*h*w][2] (TO) = (-s v, s v), s = coef * gscale / max(loss_out[1], 1): the gradient of a
//   two-class map whose per-pixel residual is (-g, g).
template <bool PAIR, typename TO>
__global__ __launch_bounds__(kYCells * kYChunks) void fss_adjoint_ypass_kernel(
    long ncell, int h, int w, int H, const float* __restrict__ rx, float coef, const float* __restrict__ loss_out,
    const float* __restrict__ gscale, TO* __restrict__ out) {
  __shared__ float part[kYChunks][kYCells];
  const int cl = threadIdx.x % kYCells, ch = threadIdx.x / kYCells;
  const long o = (long)blockIdx.x * kYCells + cl;
  float acc = 0.f;
  if (o < ncell) {
    const int j = o % w, i = (o / w) % h;
    const long p = o / ((long)w * h);
    const int ya = first_pixel(i - 1, h, H), yb = end_pixel(i, h, H);
    const int cs = (yb - ya + kYChunks - 1) / kYChunks;
    const int y0 = ya + ch * cs, y1 = min(yb, y0 + cs);
    const float* col = rx + p * H * w + j;
    for (int y = y0; y < y1; ++y) {
      bool past;
      const float wy = tap_weight(y, i, h, H, past);
      if (wy != 0.f) acc = fmaf(wy, col[(long)y * w], acc);
    }
  }
  part[ch][cl] = acc;
  __syncthreads();
  if (ch == 0 && o < ncell) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < kYChunks; ++q) v += part[q][cl];
    if constexpr (PAIR) {
      const float s = coef * (gscale ? gscale[0] : 1.f) / fmaxf(loss_out[1], 1.f);
      stf(out + 2 * o, -s * v);
      stf(out + 2 * o + 1, s * v);
    } else {
      out[o] = v;
    }
  }
}

// count[n][k] = the sum of the x-pass workgroups' pixel counts, ascending (integers: exact below 2^24)
__global__ void fss_count_kernel(int n2, int nblk, const float* __restrict__ cntpart, float* __restrict__ count) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n2) return;
  const int n = t / 2, k = t % 2;
  float v = 0.f;
  for (int b = 0; b < nblk; ++b) v += cntpart[((long)n * nblk + b) * 2 + k];
  count[t] = v;
}

int xpass_rows(int W) { return std::max(1, std::min(kXRowsMax, kXMaxFloats / W)); }

template <bool MASK>
int launch_xpass(int n, int H, int W, int w, const void* src, float* rx, float* cntpart, hipStream_t s) {
  const int R = xpass_rows(W);
  const size_t lds = (size_t)R * W * sizeof(float);
  DFM_LAUNCH(fss_adjoint_xpass_kernel<MASK>, dim3(cdiv(H, R), n), dim3(kXT), lds, s, H, W, w, R, src, rx, cntpart);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

// ------------------------------------------------------------------ weighted row sum / rank-2 outer product
constexpr int kRsCols = 64, kRsChunks = 16;

// wgt[n * cells + cell][k] = foot[n][k][cell] / ((count[n][k] + 1e-5) * S): the weight of a support
// feature row in its episode's class-k prototype (builder.py:316 and the mean over shots, 287-288)
__global__ void fss_pool_weights_kernel(long rows, int cells, float inv_s, const float* __restrict__ foot,
                                        const float* __restrict__ count, float* __restrict__ wgt) {
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (t >= rows * 2) return;
  const int k = t % 2;
  const long r = t / 2, n = r / cells, cell = r % cells;
  wgt[t] = foot[(n * 2 + k) * cells + cell] / (count[n * 2 + k] + 1e-5f) * inv_s;
}

// out[g][k][c] = sum_{r < R} coef[g R + r][k] x[g R + r][c]  (+ (sum_r tcoef[g R + r][k]) v[g][k][c])
// 64 channel lanes x 16 contiguous row chunks, each summed in ascending r, combined in ascending order.
template <typename T>
__global__ __launch_bounds__(kRsCols * kRsChunks) void fss_rowsum2_kernel(long R, int C, const T* __restrict__ x,
                                                                         long ldx, const float* __restrict__ coef,
                                                                         const float* __restrict__ tcoef,
                                                                         const float* __restrict__ v,
                                                                         float* __restrict__ out) {
  __shared__ float part[kRsChunks][2][kRsCols];
  __shared__ float tpart[kRsChunks][2];
  const int cl = threadIdx.x % kRsCols, ch = threadIdx.x / kRsCols, g = blockIdx.y;
  const int c = blockIdx.x * kRsCols + cl;
  const long cs = (R + kRsChunks - 1) / kRsChunks;
  const long r0 = g * R + ch * cs, r1 = min(g * R + R, r0 + cs);
  float a0 = 0.f, a1 = 0.f, t0 = 0.f, t1 = 0.f;
  for (long r = r0; r < r1; ++r) {
    const float xv = c < C ? ldf(x + r * ldx + c) : 0.f;
    a0 = fmaf(coef[2 * r], xv, a0);
    a1 = fmaf(coef[2 * r + 1], xv, a1);
    if (tcoef) {
      t0 += tcoef[2 * r];
      t1 += tcoef[2 * r + 1];
    }
  }
  part[ch][0][cl] = a0;
  part[ch][1][cl] = a1;
  if (cl == 0) {
    tpart[ch][0] = t0;
    tpart[ch][1] = t1;
  }
  __syncthreads();
  if (ch < 2 && c < C) {  // chunk-lane ch finishes class ch
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int q = 0; q < kRsChunks; ++q) {
      s += part[q][ch][cl];
      t += tpart[q][ch];
    }
    const long o = ((long)g * 2 + ch) * C + c;
    out[o] = tcoef ? fmaf(t, v[o], s) : s;
  }
}

// y[r][c] (+)= coef[r][0] v[g][0][c] + coef[r][1] v[g][1][c] (+ selfc[r] x[r][c]),  g = r / R
template <typename T>
__global__ void fss_outer2_kernel(long rows, long R, int C, const float* __restrict__ coef,
                                  const float* __restrict__ v, const float* __restrict__ selfc,
                                  const T* __restrict__ x, long ldx, T* __restrict__ y, long ldy, int accumulate) {
  const long n = rows * C;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int c = e % C;
    const long r = e / C, g = r / R;
    float a = coef[2 * r] * v[(g * 2) * C + c];
    a = fmaf(coef[2 * r + 1], v[(g * 2 + 1) * C + c], a);
    if (selfc) a = fmaf(selfc[r], ldf(x + r * ldx + c), a);
    if (accumulate) a += ldf(y + r * ldy + c);
    stf(y + r * ldy + c, a);
  }
}

// ------------------------------------------------------------------ cosine similarity + softmax
constexpr float kCosEps = 1e-8f;  // F.cosine_similarity clamps each norm at eps
constexpr float kSimScale = 20.f; // builder.py:319 scaler
constexpr int kSimRows = 16;      // query rows per workgroup (4 waves, one row per wave at a time)

// One wave per query row: the two dot products with the episode's prototypes and the row's squared norm
// (lanes stride the channels, xor butterfly). cos_k = q . P_k / (max(|q|, eps) max(|P_k|, eps)), so a zero
// prototype gives exactly 0; prob = softmax_k(20 cos_k / T).
template <typename T>
__global__ __launch_bounds__(256) void fss_sim_fwd_kernel(int cells, int C, const T* __restrict__ q, long ldq,
                                                          const float* __restrict__ proto, float inv_t,
                                                          float* __restrict__ prob, float* __restrict__ cosv,
                                                          float* __restrict__ qnorm, float* __restrict__ pnorm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const float* p0 = proto + (long)b * 2 * C;
  const float* p1 = p0 + C;
  float n0 = 0.f, n1 = 0.f;
  for (int c = lane; c < C; c += 64) {
    n0 = fmaf(p0[c], p0[c], n0);
    n1 = fmaf(p1[c], p1[c], n1);
  }
  n0 = fmaxf(sqrtf(wave_sum(n0)), kCosEps);
  n1 = fmaxf(sqrtf(wave_sum(n1)), kCosEps);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    pnorm[b * 2] = n0;
    pnorm[b * 2 + 1] = n1;
  }
  const int c0 = blockIdx.x * kSimRows;
  for (int cell = c0 + wave; cell < min(cells, c0 + kSimRows); cell += 4) {
    const long r = (long)b * cells + cell;
    const T* qr = q + r * ldq;
    float d0 = 0.f, d1 = 0.f, qq = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float v = ldf(qr + c);
      d0 = fmaf(v, p0[c], d0);
      d1 = fmaf(v, p1[c], d1);
      qq = fmaf(v, v, qq);
    }
    d0 = wave_sum(d0);
    d1 = wave_sum(d1);
    qq = wave_sum(qq);
    if (lane == 0) {
      const float nq = fmaxf(sqrtf(qq), kCosEps);
      const float cs0 = d0 / (nq * n0), cs1 = d1 / (nq * n1);
      const float z0 = kSimScale * cs0 * inv_t, z1 = kSimScale * cs1 * inv_t;
      const float m = fmaxf(z0, z1);
      const float e0 = expf(z0 - m), e1 = expf(z1 - m);
      const float rs = 1.f / (e0 + e1);
      prob[2 * r] = e0 * rs;
      prob[2 * r + 1] = e1 * rs;
      if (cosv) {
        cosv[2 * r] = cs0;
        cosv[2 * r + 1] = cs1;
        qnorm[r] = nq;
      }
    }
  }
}

// Per query row, from dprob: dcos_k = 20 / T * prob_k (dprob_k - sum_j prob_j dprob_j) and the
// coefficients of the two sums the backward is made of:
//   a[r][k]  = dcos_k / (|q| |P_k|)                       dq += a[r][k] P_k,  dproto_k += a[r][k] q_r
//   tc[r][k] = -dcos_k cos_k / |P_k|^2  (0 when clamped)  dproto_k += (sum_r tc[r][k]) P_k
//   sc[r]    = -sum_k dcos_k cos_k / |q|^2 (0 when clamped)  dq += sc[r] q_r
__global__ void fss_sim_bwd_coef_kernel(long rows, int cells, float inv_t, const float* __restrict__ dprob,
                                        const float* __restrict__ prob, const float* __restrict__ cosv,
                                        const float* __restrict__ qnorm, const float* __restrict__ pnorm,
                                        float* __restrict__ a, float* __restrict__ tc, float* __restrict__ sc) {
  const long r = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const long b = r / cells;
  const float pr0 = prob[2 * r], pr1 = prob[2 * r + 1];
  // two classes: prob_0 (dprob_0 - dot) = prob_0 prob_1 (dprob_0 - dprob_1), without the cancellation the
  // general form suffers when the softmax saturates
  const float dc0 = kSimScale * inv_t * pr0 * pr1 * (dprob[2 * r] - dprob[2 * r + 1]), dc1 = -dc0;
  const float nq = qnorm[r], n0 = pnorm[2 * b], n1 = pnorm[2 * b + 1];
  const float cs0 = cosv[2 * r], cs1 = cosv[2 * r + 1];
  a[2 * r] = dc0 / (nq * n0);
  a[2 * r + 1] = dc1 / (nq * n1);
  tc[2 * r] = n0 > kCosEps ? -dc0 * cs0 / (n0 * n0) : 0.f;
  tc[2 * r + 1] = n1 > kCosEps ? -dc1 * cs1 / (n1 * n1) : 0.f;
  sc[r] = nq > kCosEps ? -(dc0 * cs0 + dc1 * cs1) / (nq * nq) : 0.f;
}

// ------------------------------------------------------------------ dual-source loss
constexpr int kLossBlocks = 1024;

// z_k = alpha * up(low)[k] + (1 - alpha) * up(prob)[k] at pixel (b, y, x)
template <typename T>
DFM_INLINE void fused_logits(const T* __restrict__ low, long ldl, int h, int w, const float* __restrict__ prob,
                             int hs, int ws, int H, int W, int b, int y, int x, float alpha, float& z0, float& z1) {
  int i0, i1, j0, j1;
  float ly, lx;
  src_idx(y, h, H, i0, i1, ly);
  src_idx(x, w, W, j0, j1, lx);
  const T* r0 = low + ((long)b * h + i0) * w * ldl;
  const T* r1 = low + ((long)b * h + i1) * w * ldl;
  float a00 = (1.f - ly) * (1.f - lx), a01 = (1.f - ly) * lx, a10 = ly * (1.f - lx), a11 = ly * lx;
  const float l0 = a00 * ldf(r0 + j0 * ldl) + a01 * ldf(r0 + j1 * ldl) + a10 * ldf(r1 + j0 * ldl) +
                   a11 * ldf(r1 + j1 * ldl);
  const float l1 = a00 * ldf(r0 + j0 * ldl + 1) + a01 * ldf(r0 + j1 * ldl + 1) + a10 * ldf(r1 + j0 * ldl + 1) +
                   a11 * ldf(r1 + j1 * ldl + 1);
  src_idx(y, hs, H, i0, i1, ly);
  src_idx(x, ws, W, j0, j1, lx);
  const float* s0 = prob + ((long)b * hs + i0) * ws * 2;
  const float* s1 = prob + ((long)b * hs + i1) * ws * 2;
  a00 = (1.f - ly) * (1.f - lx); a01 = (1.f - ly) * lx; a10 = ly * (1.f - lx); a11 = ly * lx;
  const float q0 = a00 * s0[j0 * 2] + a01 * s0[j1 * 2] + a10 * s1[j0 * 2] + a11 * s1[j1 * 2];
  const float q1 = a00 * s0[j0 * 2 + 1] + a01 * s0[j1 * 2 + 1] + a10 * s1[j0 * 2 + 1] + a11 * s1[j1 * 2 + 1];
  z0 = alpha * l0 + (1.f - alpha) * q0;
  z1 = alpha * l1 + (1.f - alpha) * q1;
}

// One thread per label pixel (grid-stride): the two fused logits, the two-class CE term of a valid pixel
// (label 0 or 1; 255 and anything else is ignored) and, when gplane is given, the residual of class 1,
// softmax_1 - [label == 1] (0 on an ignored pixel). Block partials (sum, count) go to part.
template <typename T>
__global__ __launch_bounds__(256) void fss_loss_fwd_kernel(int B, int h, int w, const T* __restrict__ low, long ldl,
                                                           int hs, int ws, const float* __restrict__ prob, int H,
                                                           int W, const long long* __restrict__ label, float alpha,
                                                           float* __restrict__ gplane, float* __restrict__ part) {
  const long n = (long)B * H * W;
  float s = 0.f, cnt = 0.f;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
    const int x = p % W, y = (p / W) % H, b = p / ((long)W * H);
    const long long lab = label[p];
    float g = 0.f;
    if (lab == 0 || lab == 1) {
      float z0, z1;
      fused_logits(low, ldl, h, w, prob, hs, ws, H, W, b, y, x, alpha, z0, z1);
      const float m = fmaxf(z0, z1);
      const float e0 = __expf(z0 - m), e1 = __expf(z1 - m), se = e0 + e1;
      s += m + __logf(se) - (lab == 1 ? z1 : z0);
      cnt += 1.f;
      g = e1 / se - (lab == 1 ? 1.f : 0.f);
    }
    if (gplane) gplane[p] = g;
  }
  s = wave_sum(s);
  cnt = wave_sum(cnt);
  __shared__ float red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    part[blockIdx.x * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// (loss sum, valid count) of the block partials: lane l sums partials l, l + 64, ..., then a butterfly
__global__ void fss_loss_sum_kernel(int nblk, const float* __restrict__ part, float* __restrict__ out) {
  float s0 = 0.f, s1 = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 64) {
    s0 += part[b * 2];
    s1 += part[b * 2 + 1];
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (threadIdx.x == 0) {
    out[0] = s0;
    out[1] = s1;
  }
}

// out [B][H][W][2] float32 = the fused logits (NHWC rows)
template <typename T>
__global__ __launch_bounds__(256) void fss_fuse_fwd_kernel(int B, int h, int w, const T* __restrict__ low, long ldl,
                                                           int hs, int ws, const float* __restrict__ prob, int H,
                                                           int W, float alpha, float2* __restrict__ out) {
  const long n = (long)B * H * W;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
    const int x = p % W, y = (p / W) % H, b = p / ((long)W * H);
    float z0, z1;
    fused_logits(low, ldl, h, w, prob, hs, ws, H, W, b, y, x, alpha, z0, z1);
    out[p] = make_float2(z0, z1);
  }
}

bool grid_ok(int n, int h, int w, int H, int W) {
  return n > 0 && n <= 65535 && h > 0 && w > 0 && h <= H && w <= W && W <= kXMaxFloats;
}

}  // namespace

// ====================================================================================== entry points
/* workspace of dfm_fss_mask_footprint: the x-pass rows rx [n][2][H][w'] and the workgroups' counts */
extern "C" size_t dfm_fss_footprint_workspace(int n, int hs, int ws, int H, int W) {
  if (!grid_ok(n, hs, ws, H, W)) return 0;
  return ((size_t)n * 2 * H * ws + (size_t)n * cdiv(H, xpass_rows(W)) * 2) * sizeof(float);
}

extern "C" int dfm_fss_mask_footprint(int n, int hs, int ws, int H, int W, const long long* mask, float* foot,
                                      float* count, void* workspace, dfm_stream_t stream) {
  DFM_CHECK_ARG(mask && foot && count && workspace, "dfm_fss_mask_footprint: null pointer");
  DFM_CHECK_ARG(grid_ok(n, hs, ws, H, W),
                "dfm_fss_mask_footprint: bad shape (n=%d in [1, 65535], %dx%d <= %dx%d, W <= %d)", n, hs, ws, H, W,
                kXMaxFloats);
  DFM_CHECK_ARG((long)H * W < (1L << 24), "dfm_fss_mask_footprint: %dx%d pixels exceed the 2^24 a float32 count holds",
                H, W);
  hipStream_t s = (hipStream_t)stream;
  float* rx = (float*)workspace;
  float* cntpart = rx + (size_t)n * 2 * H * ws;
  const int nblk = (int)cdiv(H, xpass_rows(W));
  const int st = launch_xpass<true>(n, H, W, ws, mask, rx, cntpart, s);
  if (st != DFM_OK) return st;
  const long ncell = (long)n * 2 * hs * ws;
  DFM_LAUNCH((fss_adjoint_ypass_kernel<false, float>), dim3(cdiv(ncell, kYCells)), dim3(kYCells * kYChunks), 0, s,
             ncell, hs, ws, H, (const float*)rx, 1.f, (const float*)nullptr, (const float*)nullptr, foot);
  DFM_LAUNCH_CHECK();
  DFM_LAUNCH(fss_count_kernel, dim3(cdiv(2 * n, 64)), dim3(64), 0, s, 2 * n, nblk, (const float*)cntpart, count);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_fss_proto_pool_fwd(int dtype, int B, int S, int cells, int C, const void* f, long ldf_,
                                      const float* foot, const float* count, float* wgt, float* proto,
                                      dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(f && foot && count && wgt && proto, "dfm_fss_proto_pool_fwd: null pointer");
  DFM_CHECK_ARG(B > 0 && B <= 65535 && S > 0 && cells > 0 && C > 0 && ldf_ >= C,
                "dfm_fss_proto_pool_fwd: bad shape (B=%d, S=%d, cells=%d, C=%d, ld=%ld)", B, S, cells, C, ldf_);
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)B * S * cells;
  DFM_LAUNCH(fss_pool_weights_kernel, dim3(cdiv(rows * 2, 256)), dim3(256), 0, s, rows, cells, 1.f / (float)S, foot,
             count, wgt);
  DFM_LAUNCH_CHECK();
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(fss_rowsum2_kernel<T>, dim3(cdiv(C, kRsCols), B), dim3(kRsCols * kRsChunks), 0, s,
                              (long)S * cells, C, (const T*)f, ldf_, (const float*)wgt, (const float*)nullptr,
                              (const float*)nullptr, proto));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_fss_proto_pool_bwd(int dtype, int B, int S, int cells, int C, const float* wgt,
                                      const float* dproto, void* df, long lddf, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(wgt && dproto && df, "dfm_fss_proto_pool_bwd: null pointer");
  DFM_CHECK_ARG(B > 0 && S > 0 && cells > 0 && C > 0 && lddf >= C,
                "dfm_fss_proto_pool_bwd: bad shape (B=%d, S=%d, cells=%d, C=%d, ld=%ld)", B, S, cells, C, lddf);
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)B * S * cells;
  const dim3 grid((unsigned)std::min(8192L, (rows * C + 255) / 256));
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(fss_outer2_kernel<T>, grid, dim3(256), 0, s, rows, (long)S * cells, C, wgt, dproto,
                              (const float*)nullptr, (const T*)nullptr, 0L, (T*)df, lddf, 0));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_fss_sim_fwd(int dtype, int B, int cells, int C, const void* q, long ldq, const float* proto,
                               float inv_t, float* prob, float* cosv, float* qnorm, float* pnorm,
                               dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(q && proto && prob && pnorm, "dfm_fss_sim_fwd: null pointer");
  DFM_CHECK_ARG((cosv != nullptr) == (qnorm != nullptr), "dfm_fss_sim_fwd: cos and qnorm go together");
  DFM_CHECK_ARG(B > 0 && B <= 65535 && cells > 0 && C > 0 && ldq >= C && inv_t > 0.f,
                "dfm_fss_sim_fwd: bad argument (B=%d, cells=%d, C=%d, ld=%ld, 1/T=%g)", B, cells, C, ldq,
                (double)inv_t);
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(fss_sim_fwd_kernel<T>, dim3(cdiv(cells, kSimRows), B), dim3(256), 0, (hipStream_t)stream,
                              cells, C, (const T*)q, ldq, proto, inv_t, prob, cosv, qnorm, pnorm));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

/* workspace of dfm_fss_sim_bwd: the per-row coefficients a [rows][2], tc [rows][2], sc [rows] */
extern "C" size_t dfm_fss_sim_bwd_workspace(int B, int cells) {
  if (B <= 0 || cells <= 0) return 0;
  return (size_t)B * cells * 5 * sizeof(float);
}

extern "C" int dfm_fss_sim_bwd(int dtype, int B, int cells, int C, const void* q, long ldq, const float* proto,
                               float inv_t, const float* dprob, const float* prob, const float* cosv,
                               const float* qnorm, const float* pnorm, void* dq, long lddq, int accumulate,
                               float* dproto, void* workspace, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(q && proto && dprob && prob && cosv && qnorm && pnorm && dq && dproto && workspace,
                "dfm_fss_sim_bwd: null pointer");
  DFM_CHECK_ARG(B > 0 && B <= 65535 && cells > 0 && C > 0 && ldq >= C && lddq >= C && inv_t > 0.f,
                "dfm_fss_sim_bwd: bad argument (B=%d, cells=%d, C=%d, ld=%ld / %ld, 1/T=%g)", B, cells, C, ldq, lddq,
                (double)inv_t);
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)B * cells;
  float* a = (float*)workspace;
  float* tc = a + 2 * rows;
  float* sc = tc + 2 * rows;
  DFM_LAUNCH(fss_sim_bwd_coef_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, s, rows, cells, inv_t, dprob, prob, cosv,
             qnorm, pnorm, a, tc, sc);
  DFM_LAUNCH_CHECK();
  const dim3 grid((unsigned)std::min(8192L, (rows * C + 255) / 256));
  DFM_DTYPE_SWITCH(dtype, T, {
    DFM_LAUNCH(fss_rowsum2_kernel<T>, dim3(cdiv(C, kRsCols), B), dim3(kRsCols * kRsChunks), 0, s, (long)cells, C,
               (const T*)q, ldq, (const float*)a, (const float*)tc, proto, dproto);
    DFM_LAUNCH(fss_outer2_kernel<T>, grid, dim3(256), 0, s, rows, (long)cells, C, (const float*)a, proto,
               (const float*)sc, (const T*)q, ldq, (T*)dq, lddq, accumulate);
  });
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" size_t dfm_fss_loss_workspace(void) { return (size_t)kLossBlocks * 2 * sizeof(float); }

extern "C" int dfm_fss_loss_fwd(int dtype, int B, int h, int w, const void* low, long ldl, int hs, int ws,
                                const float* prob, int H, int W, const long long* label, float alpha, float* gplane,
                                float* loss_out, void* workspace, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(low && prob && label && loss_out && workspace, "dfm_fss_loss_fwd: null pointer");
  DFM_CHECK_ARG(grid_ok(B, h, w, H, W) && grid_ok(B, hs, ws, H, W) && ldl >= 2,
                "dfm_fss_loss_fwd: bad shape (B=%d, %dx%d and %dx%d <= %dx%d, ld=%ld)", B, h, w, hs, ws, H, W, ldl);
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W;
  const int nblk = (int)std::min((long)kLossBlocks, (n + 255) / 256);
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(fss_loss_fwd_kernel<T>, dim3(nblk), dim3(256), 0, s, B, h, w, (const T*)low, ldl, hs, ws,
                              prob, H, W, label, alpha, gplane, (float*)workspace));
  DFM_LAUNCH_CHECK();
  DFM_LAUNCH(fss_loss_sum_kernel, dim3(1), dim3(64), 0, s, nblk, (const float*)workspace, loss_out);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

/* workspace of dfm_fss_loss_bwd: the x-pass rows of the wider of the two grids */
extern "C" size_t dfm_fss_loss_bwd_workspace(int B, int h, int w, int hs, int ws, int H, int W) {
  if (!grid_ok(B, h, w, H, W) || !grid_ok(B, hs, ws, H, W)) return 0;
  return (size_t)B * H * std::max(w, ws) * sizeof(float);
}

extern "C" int dfm_fss_loss_bwd(int dtype_out, int B, int h, int w, int hs, int ws, int H, int W,
                                const float* gplane, const float* loss_out, const float* gscale, float alpha,
                                void* dlow, float* dprob, void* workspace, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype_out);
  DFM_CHECK_ARG(gplane && loss_out && dlow && dprob && workspace, "dfm_fss_loss_bwd: null pointer");
  DFM_CHECK_ARG(grid_ok(B, h, w, H, W) && grid_ok(B, hs, ws, H, W),
                "dfm_fss_loss_bwd: bad shape (B=%d, %dx%d and %dx%d <= %dx%d)", B, h, w, hs, ws, H, W);
  hipStream_t s = (hipStream_t)stream;
  float* rx = (float*)workspace;
  int st = launch_xpass<false>(B, H, W, w, gplane, rx, nullptr, s);
  if (st != DFM_OK) return st;
  const long nl = (long)B * h * w, ns = (long)B * hs * ws;
  DFM_DTYPE_SWITCH(dtype_out, T,
                   DFM_LAUNCH((fss_adjoint_ypass_kernel<true, T>), dim3(cdiv(nl, kYCells)), dim3(kYCells * kYChunks), 0,
                              s, nl, h, w, H, (const float*)rx, alpha, loss_out, gscale, (T*)dlow));
  DFM_LAUNCH_CHECK();
  st = launch_xpass<false>(B, H, W, ws, gplane, rx, nullptr, s);
  if (st != DFM_OK) return st;
  DFM_LAUNCH((fss_adjoint_ypass_kernel<true, float>), dim3(cdiv(ns, kYCells)), dim3(kYCells * kYChunks), 0, s, ns, hs,
             ws, H, (const float*)rx, 1.f - alpha, loss_out, gscale, dprob);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_fss_fuse_fwd(int dtype, int B, int h, int w, const void* low, long ldl, int hs, int ws,
                                const float* prob, int H, int W, float alpha, float* out, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(low && prob && out, "dfm_fss_fuse_fwd: null pointer");
  DFM_CHECK_ARG(grid_ok(B, h, w, H, W) && grid_ok(B, hs, ws, H, W) && ldl >= 2,
                "dfm_fss_fuse_fwd: bad shape (B=%d, %dx%d and %dx%d <= %dx%d, ld=%ld)", B, h, w, hs, ws, H, W, ldl);
  const long n = (long)B * H * W;
  const dim3 grid((unsigned)std::min(8192L, (n + 255) / 256));
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(fss_fuse_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, B, h, w, (const T*)low,
                              ldl, hs, ws, prob, H, W, alpha, (float2*)out));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
