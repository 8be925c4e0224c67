// libdformer_criterion.so: the focal and Tversky / Dice terms of the segmentation criterion, fused with the
// bilinear upsample of the low-resolution logits (include/dformer_criterion.h states the definitions).
//
// Forward, seg_terms_fwd_kernel: one lane per label pixel, a block inside one image. The lane interpolates
//   its class row from the 4 low-res taps into its own LDS row, turns it into the softmax in place and forms
//   its focal term. The block's per-class sums (SP, TP, SY) are column sums of those rows: wave v sums rows
//   64 v .. 64 v + 63 of column c = lane, the waves' sums are added in wave order. Block partials go to the
//   workspace; seg_terms_reduce_kernel sums them per (image, class) (one wave each: lane l takes blocks
//   l, l + 64, ..., then a butterfly), writes stats and w[c] (1 - T_bc); seg_terms_final_kernel sums those.
// Backward, seg_terms_bwd_kernel: a gather, one wave per low-res cell. The wave walks the label pixels whose
//   taps touch the cell, 64 at a time: every lane recomputes its pixel's softmax, forms
//     dz_c = F (delta_cy - p_c) + p_c (g_c - sum_k p_k g_k)
//   scaled by the pixel's tap weight on the cell into its LDS row, and lane c adds column c in row order. Every
//   output element is one fixed-order sum: no atomics, bitwise reproducible, any h <= H and w <= W.
//   A pixel touches up to 4 cells, so its softmax is recomputed up to 4 times.
// The class rows live in LDS (pitch ncls | 1, conflict-free for both the row-wise and the column-wise walk),
// not in registers: one instantiation per storage type serves every class count.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/dformer_criterion.h"

static thread_local char g_err[256] = "";

static void dfc_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* dfc_last_error(void) { return g_err; }
extern "C" int dfc_abi_version(void) { return 1; }

#define DFC_CHECK_ARG(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      dfc_set_error(__VA_ARGS__); \
      return DFC_ERR_ARG;         \
    }                             \
  } while (0)

#define DFC_INLINE __device__ __forceinline__

namespace {

constexpr int MAXC = DFC_MAX_CLASSES;

typedef uint16_t bf16_t;  // raw bfloat16 bits
struct f16_t {            // raw IEEE binary16 bits
  uint16_t bits;
};

DFC_INLINE float ldf(const float* p) { return *p; }
DFC_INLINE float ldf(const bf16_t* p) { return __uint_as_float(((uint32_t)*p) << 16); }
DFC_INLINE float ldf(const f16_t* p) { return (float)__builtin_bit_cast(_Float16, p->bits); }
DFC_INLINE void stf(float* p, float v) { *p = v; }
DFC_INLINE void stf(bf16_t* p, float v) { *p = __builtin_bit_cast(bf16_t, (__bf16)v); }
DFC_INLINE void stf(f16_t* p, float v) { p->bits = __builtin_bit_cast(uint16_t, (_Float16)v); }

DFC_INLINE float wave_sum(float v) {  // butterfly: the same order on every run
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The tap rule of F.interpolate(mode="bilinear", align_corners=False), as csrc/loss.hip states it
DFC_INLINE void src_idx(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

struct Geo {
  int B, h, w, ncls, H, W, ignore;
  int pitch;  // LDS row pitch in floats: ncls | 1
};

struct Soft {
  float q, omq, logq;  // p_y, sum of the other classes' probabilities, log p_y
};

// Pixel (y, x) of image b: row[c] <- softmax(up(logits))[c] for c < ncls; the label class's figures.
// 1 - q is the sum of the other probabilities and log q = -log1p(others / e_y): neither cancels at q -> 1.
template <typename T>
DFC_INLINE Soft pixel_softmax(const T* __restrict__ lg, const Geo& g, int b, int y, int x, int lab, float* row) {
  int h0, h1, w0, w1;
  float lh, lw;
  src_idx(y, g.h, g.H, h0, h1, lh);
  src_idx(x, g.w, g.W, w0, w1, lw);
  const T* p00 = lg + (((long)b * g.h + h0) * g.w + w0) * g.ncls;
  const T* p01 = lg + (((long)b * g.h + h0) * g.w + w1) * g.ncls;
  const T* p10 = lg + (((long)b * g.h + h1) * g.w + w0) * g.ncls;
  const T* p11 = lg + (((long)b * g.h + h1) * g.w + w1) * g.ncls;
  const float a00 = (1.f - lh) * (1.f - lw), a01 = (1.f - lh) * lw, a10 = lh * (1.f - lw), a11 = lh * lw;
  float m = -INFINITY;
  for (int c = 0; c < g.ncls; ++c) {
    const float z = a00 * ldf(p00 + c) + a01 * ldf(p01 + c) + a10 * ldf(p10 + c) + a11 * ldf(p11 + c);
    row[c] = z;
    m = fmaxf(m, z);
  }
  const float zy = row[lab] - m;
  float se = 0.f, so = 0.f, ey = 0.f;
  for (int c = 0; c < g.ncls; ++c) {
    const float e = __expf(row[c] - m);
    row[c] = e;
    se += e;
    if (c == lab) ey = e;
    else so += e;
  }
  const float inv = 1.f / se;
  for (int c = 0; c < g.ncls; ++c) row[c] *= inv;
  Soft s;
  s.q = ey * inv;
  s.omq = so * inv;
  s.logq = zy > -80.f ? -log1pf(so / ey) : zy - __logf(se);  // e_y has underflowed below -87
  return s;
}

struct FwdArgs {
  Geo g;
  const void* logits;
  const long long* label;
  const float* weight;
  float gamma;
  int has_pixel, has_region;
  int nblk;      // blocks per image
  float* part;   // [B][nblk][ncls][3]  (TP, SP, SY)
  float* lpart;  // [B][nblk][2]        (pixel-term sum, valid count)
};

template <typename T>
__global__ __launch_bounds__(256) void seg_terms_fwd_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [blockDim.x][pitch]
  __shared__ int slab[256];
  __shared__ float sw[MAXC];
  __shared__ float wpart[4][MAXC][3];
  __shared__ float red[2][4];
  const Geo& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int b = blockIdx.y;
  const long HW = (long)g.H * g.W, p = (long)blockIdx.x * blockDim.x + tid;
  if (tid < MAXC) sw[tid] = tid < g.ncls ? (a.weight ? a.weight[tid] : 1.f) : 0.f;
  __syncthreads();
  float* row = rows + tid * g.pitch;
  int lab = -1;
  if (p < HW) {
    const long long l = a.label[(long)b * HW + p];
    if (l != g.ignore && l >= 0 && l < g.ncls) lab = (int)l;
  }
  float ls = 0.f, lc = 0.f;
  if (lab >= 0) {
    const int y = (int)(p / g.W), x = (int)(p - (long)y * g.W);
    const Soft s = pixel_softmax((const T*)a.logits, g, b, y, x, lab, row);
    lc = 1.f;
    if (a.has_pixel) ls = sw[lab] * (a.gamma == 0.f ? 1.f : powf(s.omq, a.gamma)) * -s.logq;
  } else if (a.has_region) {
    for (int c = 0; c < g.ncls; ++c) row[c] = 0.f;
  }
  slab[tid] = lab;
  ls = wave_sum(ls);
  lc = wave_sum(lc);
  if (lane == 0) {
    red[0][wv] = ls;
    red[1][wv] = lc;
  }
  __syncthreads();
  const long blk = (long)b * a.nblk + blockIdx.x;
  if (tid == 0) {
    float s0 = 0.f, s1 = 0.f;
    for (int q = 0; q < nw; ++q) {
      s0 += red[0][q];
      s1 += red[1][q];
    }
    a.lpart[blk * 2] = s0;
    a.lpart[blk * 2 + 1] = s1;
  }
  if (!a.has_region) return;
  if (lane < g.ncls) {  // column `lane` of this wave's 64 rows, in row order
    float tp = 0.f, sp = 0.f, sy = 0.f;
    for (int r = wv * 64; r < wv * 64 + 64; ++r) {
      const float v = rows[r * g.pitch + lane];
      const bool own = slab[r] == lane;
      sp += v;
      tp += own ? v : 0.f;
      sy += own ? 1.f : 0.f;
    }
    wpart[wv][lane][0] = tp;
    wpart[wv][lane][1] = sp;
    wpart[wv][lane][2] = sy;
  }
  __syncthreads();
  if (tid < g.ncls) {
    float t[3] = {0.f, 0.f, 0.f};
    for (int q = 0; q < nw; ++q)
      for (int k = 0; k < 3; ++k) t[k] += wpart[q][tid][k];
    float* o = a.part + (blk * g.ncls + tid) * 3;
    o[0] = t[0];
    o[1] = t[1];
    o[2] = t[2];
  }
}

// T_bc and its two derivatives with respect to p_ic (y_i != c, y_i == c)
struct Tv {
  float T, d_other, d_own;
};
DFC_INLINE Tv tversky(float TP, float SP, float SY, float alpha, float beta, float smooth) {
  const float N = TP + smooth;
  const float D = TP + alpha * (SP - TP) + beta * (SY - TP) + smooth;
  const float iD = 1.f / D;
  Tv t;
  t.T = N * iD;
  t.d_other = -N * alpha * iD * iD;
  t.d_own = iD - N * (1.f - beta) * iD * iD;
  return t;
}

// block (b, c), one wave: c < ncls sums the image's block partials of class c; c == ncls the image's
// pixel-term partials
__global__ __launch_bounds__(64) void seg_terms_reduce_kernel(int ncls, int nblk, const float* __restrict__ part,
                                                              const float* __restrict__ lpart,
                                                              const float* __restrict__ weight, float alpha,
                                                              float beta, float smooth, int has_region,
                                                              float* __restrict__ stats, float* __restrict__ tl,
                                                              float* __restrict__ img) {
  const int b = blockIdx.x / (ncls + 1), c = blockIdx.x % (ncls + 1);
  const int lane = threadIdx.x;
  if (c == ncls) {
    float s0 = 0.f, s1 = 0.f;
    for (int k = lane; k < nblk; k += 64) {
      s0 += lpart[((long)b * nblk + k) * 2];
      s1 += lpart[((long)b * nblk + k) * 2 + 1];
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0) {
      img[b * 2] = s0;
      img[b * 2 + 1] = s1;
    }
    return;
  }
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  if (has_region) {
    for (int k = lane; k < nblk; k += 64) {
      const float* q = part + (((long)b * nblk + k) * ncls + c) * 3;
      t0 += q[0];
      t1 += q[1];
      t2 += q[2];
    }
    t0 = wave_sum(t0);
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
  }
  if (lane == 0) {
    float* s = stats + ((long)b * ncls + c) * 3;
    s[0] = t0;
    s[1] = t1;
    s[2] = t2;
    tl[(long)b * ncls + c] =
        has_region ? (weight ? weight[c] : 1.f) * (1.f - tversky(t0, t1, t2, alpha, beta, smooth).T) : 0.f;
  }
}

// one wave: out = (pixel-term sum, valid count, L_reg)
__global__ __launch_bounds__(64) void seg_terms_final_kernel(int B, int ncls, const float* __restrict__ tl,
                                                             const float* __restrict__ img,
                                                             float* __restrict__ out) {
  const int lane = threadIdx.x;
  float s0 = 0.f, s1 = 0.f, r = 0.f;
  for (int b = lane; b < B; b += 64) {
    s0 += img[b * 2];
    s1 += img[b * 2 + 1];
  }
  for (long k = lane; k < (long)B * ncls; k += 64) r += tl[k];
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  r = wave_sum(r);
  if (lane == 0) {
    out[0] = s0;
    out[1] = s1;
    out[2] = r / ((float)B * (float)ncls);
  }
}

// Output indices [lo, hi) that can touch low-res index i: a pixel does iff floor(src) is i - 1 or i, that
// is (i - 0.5) out / in - 0.5 <= dst < (i + 1.5) out / in - 0.5; one index of margin either side for the
// rounding of src_idx, then narrowed with src_idx itself (taps are monotone in dst).
DFC_INLINE void touch_range(int i, int in, int out, int& lo, int& hi) {
  const float inv = (float)out / (float)in;
  lo = max(0, (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1);
  hi = min(out, (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 2);
  int i0, i1;
  float l1;
  for (; lo < hi; ++lo) {
    src_idx(lo, in, out, i0, i1, l1);
    if (i0 == i || i1 == i) break;
  }
  for (; hi > lo; --hi) {
    src_idx(hi - 1, in, out, i0, i1, l1);
    if (i0 == i || i1 == i) break;
  }
}

DFC_INLINE float tap_weight(int dst, int i, int in, int out) {
  int i0, i1;
  float l1;
  src_idx(dst, in, out, i0, i1, l1);
  return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

struct BwdArgs {
  Geo g;
  const void* logits;
  const long long* label;
  const float* weight;
  const float* stats;
  const float* out;
  const float* gscale;
  float gamma, alpha, beta, smooth, region_weight;
  int has_pixel, has_region;
  void* dlogits;
};

template <typename T>
__global__ __launch_bounds__(256) void seg_terms_bwd_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rows[];  // [waves][64][pitch]
  __shared__ float sw[MAXC];
  __shared__ float coef[MAXC][2];  // gscale region_weight (-w[c] / (B C)) dT_bc/dp_ic for y_i != c, y_i == c
  const Geo& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int b = blockIdx.y;
  const float gs = a.gscale ? a.gscale[0] : 1.f;
  if (tid < MAXC) {
    const float wc = tid < g.ncls ? (a.weight ? a.weight[tid] : 1.f) : 0.f;
    sw[tid] = wc;
    float c0 = 0.f, c1 = 0.f;
    if (a.has_region && tid < g.ncls) {
      const float* s = a.stats + ((long)b * g.ncls + tid) * 3;
      const Tv t = tversky(s[0], s[1], s[2], a.alpha, a.beta, a.smooth);
      const float k = gs * a.region_weight * -wc / ((float)g.B * (float)g.ncls);
      c0 = k * t.d_other;
      c1 = k * t.d_own;
    }
    coef[tid][0] = c0;
    coef[tid][1] = c1;
  }
  __syncthreads();
  const float pixscale = a.has_pixel ? gs / fmaxf(a.out[1], 1.f) : 0.f;
  const int cell = blockIdx.x * nw + wv;
  const bool live = cell < g.h * g.w;
  const int i = live ? cell / g.w : 0, j = live ? cell - i * g.w : 0;
  int ylo = 0, yhi = 0, xlo = 0, xhi = 0;
  if (live) {
    touch_range(i, g.h, g.H, ylo, yhi);
    touch_range(j, g.w, g.W, xlo, xhi);
  }
  const int nx = xhi - xlo, npx = (yhi - ylo) * nx;
  float* wrows = rows + wv * 64 * g.pitch;
  float* row = wrows + lane * g.pitch;
  float acc = 0.f;  // lane c: dlogits[b][i][j][c]
  for (int base = 0;; base += 64) {
    const bool more = base < npx;
    if (!__syncthreads_or(more)) break;  // every wave of the block has walked its cell's pixels
    if (more) {
      const int k = base + lane;
      int lab = -1, y = 0, x = 0;
      float wgt = 0.f;
      if (k < npx) {
        y = ylo + k / nx;
        x = xlo + k % nx;
        wgt = tap_weight(y, i, g.h, g.H) * tap_weight(x, j, g.w, g.W);
        if (wgt != 0.f) {
          const long long l = a.label[((long)b * g.H + y) * g.W + x];
          if (l != g.ignore && l >= 0 && l < g.ncls) lab = (int)l;
        }
      }
      if (lab >= 0) {
        const Soft s = pixel_softmax((const T*)a.logits, g, b, y, x, lab, row);
        float F = -1.f;  // d(focal term) / dq times q, over w[y]
        if (a.gamma != 0.f) {
          // gamma q (1-q)^(gamma-1) log q - (1-q)^gamma, the first term as (1-q)^gamma (log q / (1-q)):
          // log q / (1-q) -> -1 at q -> 1, where (1-q)^(gamma-1) alone overflows for gamma < 1
          const float pw = powf(s.omq, a.gamma);
          F = (s.omq > 0.f ? a.gamma * s.q * pw * (s.logq / s.omq) : 0.f) - pw;
        }
        F *= pixscale * sw[lab];
        float dot = 0.f;
        if (a.has_region)
          for (int c = 0; c < g.ncls; ++c) dot += row[c] * coef[c][c == lab];
        for (int c = 0; c < g.ncls; ++c) {
          const float pc = row[c];
          float dz = F * ((c == lab ? 1.f : 0.f) - pc);
          if (a.has_region) dz += pc * (coef[c][c == lab] - dot);
          row[c] = wgt * dz;
        }
      } else {
        for (int c = 0; c < g.ncls; ++c) row[c] = 0.f;
      }
    }
    __syncthreads();
    if (more && lane < g.ncls) {
      const int nr = min(64, npx - base);
      for (int r = 0; r < nr; ++r) acc += wrows[r * g.pitch + lane];
    }
  }
  if (live && lane < g.ncls) stf((T*)a.dlogits + ((long)b * g.h * g.w + cell) * g.ncls + lane, acc);
}

// threads per block of both kernels: their LDS rows (threads x pitch floats) plus the static arrays stay
// under 64 KB
int block_threads(int ncls) { return ncls > 56 ? 128 : 256; }

int launch_error(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return DFC_OK;
  dfc_set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
  return DFC_ERR_LAUNCH;
}

}  // namespace

#define DFC_CHECK_COMMON(fn)                                                                                      \
  DFC_CHECK_ARG(dtype == DFC_F32 || dtype == DFC_BF16 || dtype == DFC_F16, "%s: unsupported dtype %d", fn, dtype); \
  DFC_CHECK_ARG(B > 0 && B <= DFC_MAX_BATCH, "%s: batch %d outside 1..%d", fn, B, DFC_MAX_BATCH);                  \
  DFC_CHECK_ARG(ncls > 0 && ncls <= DFC_MAX_CLASSES, "%s: ncls %d outside 1..%d", fn, ncls, DFC_MAX_CLASSES);      \
  DFC_CHECK_ARG(h > 0 && w > 0 && H > 0 && W > 0 && H <= DFC_MAX_DIM && W <= DFC_MAX_DIM,                          \
                "%s: sizes %d x %d -> %d x %d outside 1..%d", fn, h, w, H, W, DFC_MAX_DIM);                        \
  DFC_CHECK_ARG(h <= H && w <= W, "%s: %d x %d -> %d x %d is not an upsampling", fn, h, w, H, W);                  \
  DFC_CHECK_ARG(logits && label && desc, "%s: null logits, label or desc", fn);                                    \
  DFC_CHECK_ARG(desc->gamma >= 0.f && std::isfinite(desc->gamma), "%s: gamma %g is negative or not finite", fn,         \
                (double)desc->gamma);                                                                              \
  if (desc->has_region) {                                                                                          \
    DFC_CHECK_ARG(desc->smooth > 0.f, "%s: smooth %g must be > 0", fn, (double)desc->smooth);                      \
    DFC_CHECK_ARG(desc->alpha >= 0.f && desc->beta >= 0.f && desc->alpha + desc->beta > 0.f,                       \
                  "%s: alpha %g, beta %g must be >= 0 with a sum > 0", fn, (double)desc->alpha,                    \
                  (double)desc->beta);                                                                             \
  }

static Geo make_geo(int B, int h, int w, int ncls, int H, int W, int ignore) {
  Geo g;
  g.B = B, g.h = h, g.w = w, g.ncls = ncls, g.H = H, g.W = W, g.ignore = ignore;
  g.pitch = ncls | 1;
  return g;
}

extern "C" size_t dfc_seg_terms_workspace(int B, int h, int w, int ncls, int H, int W) {
  if (B <= 0 || B > DFC_MAX_BATCH || h <= 0 || w <= 0 || ncls <= 0 || ncls > DFC_MAX_CLASSES || H <= 0 || W <= 0 ||
      H > DFC_MAX_DIM || W > DFC_MAX_DIM)
    return 0;
  const long nt = block_threads(ncls), nblk = ((long)H * W + nt - 1) / nt;
  return (size_t)((long)B * nblk * (ncls * 3 + 2) + (long)B * ncls + (long)B * 2) * sizeof(float);
}

extern "C" int dfc_seg_terms_fwd(int dtype, int B, int h, int w, int ncls, const void* logits, int H, int W,
                                 const void* label, int ignore, const float* weight, const DfcTermsDesc* desc,
                                 void* workspace, float* stats, float* out, dfc_stream_t stream) {
  DFC_CHECK_COMMON("dfc_seg_terms_fwd");
  DFC_CHECK_ARG(workspace && stats && out, "dfc_seg_terms_fwd: null workspace, stats or out");
  hipStream_t s = (hipStream_t)stream;
  const int nt = block_threads(ncls);
  const long nblk = ((long)H * W + nt - 1) / nt;
  FwdArgs a;
  a.g = make_geo(B, h, w, ncls, H, W, ignore);
  a.logits = logits;
  a.label = (const long long*)label;
  a.weight = weight;
  a.gamma = desc->gamma;
  a.has_pixel = desc->has_pixel != 0, a.has_region = desc->has_region != 0;
  a.nblk = (int)nblk;
  a.part = (float*)workspace;
  a.lpart = a.part + (long)B * nblk * ncls * 3;
  float* tl = a.lpart + (long)B * nblk * 2;
  float* img = tl + (long)B * ncls;
  const size_t lds = (size_t)nt * a.g.pitch * sizeof(float);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (dtype == DFC_F32) hipLaunchKernelGGL(seg_terms_fwd_kernel<float>, grid, dim3(nt), lds, s, a);
  else if (dtype == DFC_BF16) hipLaunchKernelGGL(seg_terms_fwd_kernel<bf16_t>, grid, dim3(nt), lds, s, a);
  else hipLaunchKernelGGL(seg_terms_fwd_kernel<f16_t>, grid, dim3(nt), lds, s, a);
  if (int e = launch_error("dfc_seg_terms_fwd")) return e;
  hipLaunchKernelGGL(seg_terms_reduce_kernel, dim3((unsigned)(B * (ncls + 1))), dim3(64), 0, s, ncls, (int)nblk,
                     (const float*)a.part, (const float*)a.lpart, weight, desc->alpha, desc->beta, desc->smooth,
                     a.has_region, stats, tl, img);
  if (int e = launch_error("dfc_seg_terms_fwd")) return e;
  hipLaunchKernelGGL(seg_terms_final_kernel, dim3(1), dim3(64), 0, s, B, ncls, (const float*)tl, (const float*)img,
                     out);
  return launch_error("dfc_seg_terms_fwd");
}

extern "C" int dfc_seg_terms_bwd(int dtype, int B, int h, int w, int ncls, const void* logits, int H, int W,
                                 const void* label, int ignore, const float* weight, const DfcTermsDesc* desc,
                                 const float* stats, const float* out, const float* gscale, float region_weight,
                                 void* dlogits, dfc_stream_t stream) {
  DFC_CHECK_COMMON("dfc_seg_terms_bwd");
  DFC_CHECK_ARG(stats && out && dlogits, "dfc_seg_terms_bwd: null stats, out or dlogits");
  DFC_CHECK_ARG(region_weight >= 0.f && std::isfinite(region_weight),
                "dfc_seg_terms_bwd: region_weight %g is negative or not finite", (double)region_weight);
  hipStream_t s = (hipStream_t)stream;
  const int nt = block_threads(ncls), nw = nt / 64;
  BwdArgs a;
  a.g = make_geo(B, h, w, ncls, H, W, ignore);
  a.logits = logits;
  a.label = (const long long*)label;
  a.weight = weight;
  a.stats = stats;
  a.out = out;
  a.gscale = gscale;
  a.gamma = desc->gamma, a.alpha = desc->alpha, a.beta = desc->beta, a.smooth = desc->smooth;
  a.region_weight = region_weight;
  a.has_pixel = desc->has_pixel != 0, a.has_region = desc->has_region != 0;
  a.dlogits = dlogits;
  const size_t lds = (size_t)nt * a.g.pitch * sizeof(float);
  const dim3 grid((unsigned)(((long)h * w + nw - 1) / nw), (unsigned)B);
  if (dtype == DFC_F32) hipLaunchKernelGGL(seg_terms_bwd_kernel<float>, grid, dim3(nt), lds, s, a);
  else if (dtype == DFC_BF16) hipLaunchKernelGGL(seg_terms_bwd_kernel<bf16_t>, grid, dim3(nt), lds, s, a);
  else hipLaunchKernelGGL(seg_terms_bwd_kernel<f16_t>, grid, dim3(nt), lds, s, a);
  return launch_error("dfc_seg_terms_bwd");
}
