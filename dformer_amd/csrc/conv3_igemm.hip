// UPerNet head kernels (models/decoders/UPernet.py): the implicit-GEMM 3x3 stride-1 pad-1 conv on NHWC rows
// (forward = input gradient kernel, weight gradient) and the pyramid pooling of the PPM.
//
// The conv is the MFMA GEMM of gemm_impl.h (LDS staging, fragments, epilogue, split-K combine) with the
// operand loader replaced: the operand dfm_conv3s1_im2col would write,
//   cols[p][tap*Cin + c] = x[nbr(p, tap)][c]   (zero outside the image),
// is gathered from x while the tile is staged, so nothing of size P x 9*Cin is ever allocated.
//   forward / dgrad  y = cols @ wp^T : A gathered k-contiguous (a thread's tile rows are fixed for the whole
//                    k-loop: per row one 9-bit tap-validity mask; per k-slice only tap = k / Cin moves),
//                    B = the packed weight, k-contiguous
//   wgrad            dwp = dy^T @ cols : A = dy row-contiguous, B gathered row-contiguous (a thread's tile
//                    columns, i.e. (tap, c), are fixed; the pixel of its row advances by BK per k-slice and
//                    its (x, y) is stepped without a division); split-K over pixels, fixed-order combine;
//                    the bias gradient is the virtual all-ones column after the last tap
// Cin % 8 == 0 keeps every 16-byte vector inside one tap whether or not the k-slice divides Cin.
#include "gemm_impl.h"

namespace {

struct Conv3Args {
  GemmArgs g;        // A = x (fwd) / dy (wgrad), B = wp (fwd) / x (wgrad), M / N / K of the GEMM
  int H, W, Cin;     // image size and channels of the gathered operand
  long ldx;          // row stride of the gathered operand
  float inv_cin;     // fwd: tap = floor((k + 0.5) / Cin) in float (exact: k < 2^20, see conv3_tap)
  int sx, sy;        // wgrad: BK pixels further is (x + sx [carry into y], y + sy) mod (W, H)
};

// tap of packed column k (0 <= k < 2^20, Cin >= 8): (k + 0.5) / Cin is at least 0.5 / Cin away from an
// integer, far more than the rounding of one float multiply, so the truncation is floor(k / Cin)
DFM_INLINE int conv3_tap(int k, float inv_cin) { return (int)(((float)k + 0.5f) * inv_cin); }

template <typename T, int TM, int TN, int WM, int WN, int BK, bool AK, bool BKC, int LDA, int LDB>
DFM_INLINE void conv3_mma(float4_t (&acc)[TM][TN], const T* la, const T* lb, int wm, int wn, int lane) {
  constexpr int KSTEP = Mf<T>::KSTEP;
#pragma unroll
  for (int ks = 0; ks < BK; ks += KSTEP) {
    if constexpr (sizeof(T) == 2) {
      bf16x8_t fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = frag_bf16<AK, LDA>((const bf16_t*)la, wm * WM + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = frag_bf16<BKC, LDB>((const bf16_t*)lb, wn * WN + j * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mma16<T>(fa[i], fb[j], acc[i][j]);
    } else {
      float fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = frag_f32<AK, LDA>((const float*)la, wm * WM + i * 16, ks, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = frag_f32<BKC, LDB>((const float*)lb, wn * WN + j * 16, ks, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
}

// ---------------------------------------------------------------- forward / input gradient
template <typename T, int BM, int BN, int NW, int WAVES_M, int BK>
__global__ __launch_bounds__(64 * NW) void conv3_igemm_fwd_kernel(Conv3Args c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmArgs& a = c.g;
  constexpr int NT = 64 * NW;
  constexpr int WAVES_N = NW / WAVES_M;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 16, TN = WN / 16;
  using GA = TileGeom<T, BM, BK, true, NT>;
  using GB = TileGeom<T, BN, BK, true, NT>;
  constexpr int VEC = GA::VEC;
  static_assert(GA::TOTAL % NT == 0, "every thread stages the same number of A vectors");
  T* const lds_base = reinterpret_cast<T*>(smem);
#define LDS_A(i) (lds_base + (i) * GA::ELEMS)
#define LDS_B(i) (lds_base + 2 * GA::ELEMS + (i) * GB::ELEMS)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid / WAVES_N, wn = wid % WAVES_N;
  // consecutive (XCD-local) blocks walk the column tiles of one row tile: its gathered rows stay in L2
  const int lid = xcd_lid(blockIdx.x, gridDim.x);
  const int bm = (lid / a.tiles_n) * BM, bn = (lid % a.tiles_n) * BN;
  const T* X = (const T*)a.A;
  const T* Wp = (const T*)a.B;
  const int H = c.H, W = c.W, Cin = c.Cin;

  // this thread's A vectors: tile row (a pixel) and k offset are the same in every k-slice
  long rowoff[GA::NVEC];
  unsigned mask[GA::NVEC];  // bit tap: nbr(p, tap) is inside the image (0 for rows past the last pixel)
  int kc[GA::NVEC];
#pragma unroll
  for (int i = 0; i < GA::NVEC; ++i) {
    const int v = threadIdx.x + i * NT;
    const int p = bm + v / (BK / VEC);
    kc[i] = (v % (BK / VEC)) * VEC;
    rowoff[i] = (long)p * c.ldx;
    unsigned m = 0;
    if (p < a.M) {
      const int px = p % W, py = (p / W) % H;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
        m |= (unsigned)(yy >= 0 && yy < H && xx >= 0 && xx < W) << t;
      }
    }
    mask[i] = m;
  }
  auto load = [&](uint4* xa, uint4* xb, int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < GA::NVEC; ++i) {
      const int k = k0 + kc[i];
      const int tap = conv3_tap(k, c.inv_cin);  // >= 9 past K: no mask bit, zero fill
      const int ch = k - tap * Cin;
      const int dy = ((tap * 11) >> 5) - 1, dx = tap - 3 * (dy + 1) - 1;
      uint4 u = make_uint4(0, 0, 0, 0);
      if ((mask[i] >> tap) & 1u) u = *reinterpret_cast<const uint4*>(X + rowoff[i] + (long)(dy * W + dx) * c.ldx + ch);
      xa[i] = u;
    }
    stage_load<T, BN, BK, true, NT>(xb, Wp, a.ldb, bn, k0, a.N, a.K, true);
  };
  auto store = [&](const uint4* xa, const uint4* xb, int buf) {
    stage_store<T, BM, BK, true, NT>(xa, LDS_A(buf));
    stage_store<T, BN, BK, true, NT>(xb, LDS_B(buf));
  };

  float4_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.K + BK - 1) / BK;
  uint4 ra[GA::NVEC], rb[GB::NVEC];
  load(ra, rb, 0);
  store(ra, rb, 0);
  lds_barrier();
  int cur = 0;
  for (int kt = 0; kt + 1 < nk; ++kt) {  // slice kt+1 is requested while slice kt is multiplied
    load(ra, rb, kt + 1);
    conv3_mma<T, TM, TN, WM, WN, BK, true, true, GA::LD, GB::LD>(acc, LDS_A(cur), LDS_B(cur), wm, wn, lane);
    store(ra, rb, cur ^ 1);
    lds_barrier();
    cur ^= 1;
  }
  conv3_mma<T, TM, TN, WM, WN, BK, true, true, GA::LD, GB::LD>(acc, LDS_A(cur), LDS_B(cur), wm, wn, lane);
  lds_barrier();  // the epilogue reuses the operand LDS
#undef LDS_A
#undef LDS_B
  gemm_epilogue<T, BM, BN, NW, WAVES_M>(a, acc, smem, bm, bn, 0, 0);
}

// ---------------------------------------------------------------- weight gradient
template <typename T, int BM, int BN, int NW, int WAVES_M, int BK>
__global__ __launch_bounds__(64 * NW) void conv3_igemm_wgrad_kernel(Conv3Args c) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemmArgs& a = c.g;
  constexpr int NT = 64 * NW;
  constexpr int WAVES_N = NW / WAVES_M;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;
  constexpr int TM = WM / 16, TN = WN / 16;
  using GA = TileGeom<T, BM, BK, false, NT>;
  using GB = TileGeom<T, BN, BK, false, NT>;
  constexpr int VEC = GB::VEC;
  static_assert(GB::TOTAL % NT == 0, "every thread stages the same number of B vectors");
  T* const lds_base = reinterpret_cast<T*>(smem);
#define LDS_A(i) (lds_base + (i) * GA::ELEMS)
#define LDS_B(i) (lds_base + 2 * GA::ELEMS + (i) * GB::ELEMS)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid / WAVES_N, wn = wid % WAVES_N;
  // the tiles of one split-K slice, which read the same pixels, run on one XCD
  const int lid = xcd_lid(blockIdx.x, gridDim.x);
  const int ntile = a.tiles_m * a.tiles_n;
  const int tile = lid % ntile, split = lid / ntile;
  const int bm = (tile % a.tiles_m) * BM, bn = (tile / a.tiles_m) * BN;
  const int kper = ((a.K + a.splits - 1) / a.splits + BK - 1) / BK * BK;
  const int kbeg = split * kper;
  const int kend = min(a.K, kbeg + kper);
  const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
  const T* DY = (const T*)a.A;
  const T* X = (const T*)a.B;
  const int H = c.H, W = c.W, Cin = c.Cin;

  // this thread's B vectors: the packed columns n .. n+VEC-1 (one tap, consecutive channels) are the same in
  // every k-slice; the pixel of its tile row moves BK pixels per slice
  int kind[GB::NVEC];  // 0: past the last column, 1: gathered, 2: the virtual ones column (its first element)
  int chan[GB::NVEC], dy[GB::NVEC], dx[GB::NVEC], px[GB::NVEC], py[GB::NVEC], pp[GB::NVEC];
#pragma unroll
  for (int i = 0; i < GB::NVEC; ++i) {
    const int v = threadIdx.x + i * NT;
    const int n = bn + (v % (BN / VEC)) * VEC;
    const int tap = n / Cin;
    kind[i] = n < a.N ? 1 : (n == a.N && a.colsum != nullptr ? 2 : 0);
    chan[i] = n - tap * Cin;
    dy[i] = tap / 3 - 1;
    dx[i] = tap % 3 - 1;
    pp[i] = kbeg + v / (BN / VEC);
    px[i] = pp[i] % W;
    py[i] = (pp[i] / W) % H;
  }
  auto load = [&](uint4* xa, uint4* xb, int kt) {  // called for kt = 0, 1, 2, ... in order
    stage_load<T, BM, BK, false, NT>(xa, DY, a.lda, bm, kbeg + kt * BK, a.M, kend, true);
#pragma unroll
    for (int i = 0; i < GB::NVEC; ++i) {
      uint4 u = make_uint4(0, 0, 0, 0);
      const int p = pp[i];
      if (p < kend) {
        const int yy = py[i] + dy[i], xx = px[i] + dx[i];
        if (kind[i] == 1) {
          if (yy >= 0 && yy < H && xx >= 0 && xx < W)
            u = *reinterpret_cast<const uint4*>(X + ((long)p + dy[i] * W + dx[i]) * c.ldx + chan[i]);
        } else if (kind[i] == 2) {
          u.x = one_bits<T>();
        }
      }
      xb[i] = u;
      pp[i] = p + BK;
      int nx = px[i] + c.sx, ny = py[i] + c.sy;
      if (nx >= W) nx -= W, ++ny;
      if (ny >= H) ny -= H;
      px[i] = nx;
      py[i] = ny;
    }
  };
  auto store = [&](const uint4* xa, const uint4* xb, int buf) {
    stage_store<T, BM, BK, false, NT>(xa, LDS_A(buf));
    stage_store<T, BN, BK, false, NT>(xb, LDS_B(buf));
  };

  float4_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

  if (nk > 0) {
    uint4 ra[GA::NVEC], rb[GB::NVEC];
    load(ra, rb, 0);
    store(ra, rb, 0);
    lds_barrier();
    int cur = 0;
    for (int kt = 0; kt + 1 < nk; ++kt) {
      load(ra, rb, kt + 1);
      conv3_mma<T, TM, TN, WM, WN, BK, false, false, GA::LD, GB::LD>(acc, LDS_A(cur), LDS_B(cur), wm, wn, lane);
      store(ra, rb, cur ^ 1);
      lds_barrier();
      cur ^= 1;
    }
    conv3_mma<T, TM, TN, WM, WN, BK, false, false, GA::LD, GB::LD>(acc, LDS_A(cur), LDS_B(cur), wm, wn, lane);
    lds_barrier();
  }
#undef LDS_A
#undef LDS_B
  gemm_epilogue<T, BM, BN, NW, WAVES_M>(a, acc, smem, bm, bn, 0, split);
}

// wpt[c][tap*Cout + o] = w[o][c][8 - tap]
template <typename To>
__global__ void weight_pack_dgrad_kernel(int Cout, int Cin, const float* __restrict__ w, To* __restrict__ wpt) {
  const long kp = 9L * Cout;
  const long n = (long)Cin * kp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i % kp);
    const long ci = i / kp;
    const int tap = k / Cout, o = k - tap * Cout;
    stf(wpt + i, w[((long)o * Cin + ci) * 9 + (8 - tap)]);
  }
}

// ---------------------------------------------------------------- pyramid pooling
struct PpmScales {
  int s[4];
  int off[5];  // off[k] = sum_{j<k} s[j]^2
  int n;
};

DFM_INLINE int bin_lo(int i, int n, int s) { return (i * n) / s; }
DFM_INLINE int bin_hi(int i, int n, int s) { return ((i + 1) * n + s - 1) / s; }

// One block per output bin and 32 channel vectors: 8 row groups walk the bin's pixels (group g takes pixels
// g, g + 8, ...) and meet in LDS in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void ppm_pool_fwd_kernel(int B, int H, int W, int C, PpmScales sc,
                                                          const T* __restrict__ x, long ldx, T* __restrict__ y,
                                                          long ldy) {
  __shared__ float red[8][32][8];
  int bin = blockIdx.x;  // scale-major row of y
  int k = 0;
#pragma unroll
  for (int q = 1; q < 4; ++q)
    if (q < sc.n && bin >= B * sc.off[q]) k = q;
  const int s = sc.s[k];
  const int local = bin - B * sc.off[k];
  const int b = local / (s * s), ij = local % (s * s);
  const int i = ij / s, j = ij % s;
  const int y0 = bin_lo(i, H, s), y1 = bin_hi(i, H, s), x0 = bin_lo(j, W, s), x1 = bin_hi(j, W, s);
  const int bw = x1 - x0, npix = (y1 - y0) * bw;
  const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int c8 = blockIdx.y * 32 + cl;
  const bool on = c8 * 8 < C;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (on) {
    for (int q = g; q < npix; q += 8) {
      const int yy = y0 + q / bw, xx = x0 + q % bw;
      float v[8];
      ld8<T>(x + (((long)b * H + yy) * W + xx) * ldx + c8 * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[g][cl][e] = acc[e];
  __syncthreads();
  if (g == 0 && on) {
    const float inv = 1.0f / (float)npix;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = red[0][cl][e];
#pragma unroll
      for (int r = 1; r < 8; ++r) t += red[r][cl][e];
      acc[e] = t * inv;
    }
    st8<T>(y + (long)bin * ldy + c8 * 8, acc);
  }
}

// One thread per input pixel and 8 channels: the bins that hold the pixel, scales and bins in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void ppm_pool_bwd_kernel(int B, int H, int W, int C, PpmScales sc,
                                                          const T* __restrict__ dy, long lddy, T* __restrict__ dx,
                                                          long lddx, int accumulate) {
  const int cv = C >> 3;
  const long n = (long)B * H * W * cv;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(t % cv) * 8;
    const long p = t / cv;
    const int xx = (int)(p % W);
    const long r = p / W;
    const int yy = (int)(r % H);
    const int b = (int)(r / H);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int k = 0; k < sc.n; ++k) {
      const int s = sc.s[k];
      for (int i = 0; i < s; ++i) {
        const int y0 = bin_lo(i, H, s), y1 = bin_hi(i, H, s);
        if (yy < y0 || yy >= y1) continue;
        for (int j = 0; j < s; ++j) {
          const int x0 = bin_lo(j, W, s), x1 = bin_hi(j, W, s);
          if (xx < x0 || xx >= x1) continue;
          const float inv = 1.0f / (float)((y1 - y0) * (x1 - x0));
          float v[8];
          ld8<T>(dy + ((long)B * sc.off[k] + ((long)b * s + i) * s + j) * lddy + c0, v);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = fmaf(v[e], inv, acc[e]);
        }
      }
    }
    T* dp = dx + p * lddx + c0;
    if (accumulate) {
      float o[8];
      ld8<T>(dp, o);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += o[e];
    }
    st8<T>(dp, acc);
  }
}

// ---------------------------------------------------------------- host
template <typename T, int BM, int BN, int NW, int WM_, int BK>
size_t conv3_lds(bool kc) {
  using GA = TileGeom<T, BM, BK, true, 64 * NW>;
  using GB = TileGeom<T, BN, BK, true, 64 * NW>;
  using RA = TileGeom<T, BM, BK, false, 64 * NW>;
  using RB = TileGeom<T, BN, BK, false, 64 * NW>;
  const size_t lds_op = (size_t)2 * (kc ? GA::ELEMS + GB::ELEMS : RA::ELEMS + RB::ELEMS) * sizeof(T);
  constexpr int RP = (128 * NW / (BN / 8)) < BM ? (128 * NW / (BN / 8)) : BM;  // epilogue rows per pass
  const size_t lds_c = (size_t)RP * (BN + 4) * sizeof(float);
  return lds_op > lds_c ? lds_op : lds_c;
}

template <typename T, int BM, int BN, int NW, int WM_>
int conv3_fwd_launch(Conv3Args& c, hipStream_t s) {
  constexpr int BK = sizeof(T) == 2 ? 64 : 32;
  auto kern = conv3_igemm_fwd_kernel<T, BM, BN, NW, WM_, BK>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  c.g.tiles_m = cdiv(c.g.M, BM);
  c.g.tiles_n = cdiv(c.g.N, BN);
  DFM_LAUNCH(kern, dim3((unsigned)c.g.tiles_m * c.g.tiles_n), dim3(64 * NW), (conv3_lds<T, BM, BN, NW, WM_, BK>(true)),
             s, c);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

template <typename T>
int conv3_fwd_typed(int B, int H, int W, int Cin, int Cout, const void* x, long ldx, const void* wp,
                    const float* bias, void* y, long ldy, int accumulate, hipStream_t s) {
  Conv3Args c{};
  GemmArgs& a = c.g;
  a.A = x; a.B = wp; a.C = y;
  a.M = B * H * W; a.N = Cout; a.K = 9 * Cin; a.batch = 1; a.splits = 1;
  a.Nw = Cout; a.ldw = (Cout + 7) & ~7;
  a.lda = ldx; a.ldb = 9L * Cin; a.ldc = ldy;
  a.alpha = 1.0f; a.beta = accumulate ? 1.0f : 0.0f;
  a.bias = bias;
  a.rps = 1;
  a.ala = a.alb = 1;
  a.vec_ok = 1;  // y is 16-byte aligned with ldy % 8 == 0 (checked by the entry point)
  c.H = H; c.W = W; c.Cin = Cin; c.ldx = ldx;
  c.inv_cin = 1.0f / (float)Cin;
  if (Cout <= 32) return conv3_fwd_launch<T, 128, 32, 4, 4>(c, s);
  if (Cout <= 64) return conv3_fwd_launch<T, 128, 64, 4, 2>(c, s);
  return conv3_fwd_launch<T, 128, 128, 8, 2>(c, s);
}

// Split-K of the weight gradient: about 512 blocks (two per CU), at least 512 pixels per split.
int wgrad_splits(long P, int Cin, int Cout, int bias_grad) {
  const long tiles = (long)cdiv(Cout, 128) * cdiv(9L * Cin + (bias_grad ? 1 : 0), 128);
  long s = std::min((512 + tiles - 1) / tiles, P / 512);
  return (int)std::max(1L, std::min(s, 64L));
}

// The split-K combine of the weight gradient: splitk_reduce_block under a name of its own, so that a
// launch trace tells it from dfm_gemm's combine (this translation unit would otherwise hold a second
// kernel called splitk_reduce_kernel<T, G>).
template <typename T, int G>
__global__ __launch_bounds__(256) void conv3_splitk_reduce_kernel(GemmArgs a) {
  splitk_reduce_block<T, G>(a, blockIdx.x);
}

template <typename T>
int conv3_wgrad_typed(int B, int H, int W, int Cin, int Cout, const void* dy, long lddy, const void* x, long ldx,
                      float* dwp, float* db, void* ws, hipStream_t s) {
  constexpr int BM = 128, BN = 128, NW = 8, WM_ = 2, BK = sizeof(T) == 2 ? 64 : 32;
  Conv3Args c{};
  GemmArgs& a = c.g;
  a.A = dy; a.B = x; a.C = dwp; a.ws = (float*)ws;
  a.M = Cout; a.N = 9 * Cin; a.K = B * H * W; a.batch = 1;
  a.splits = wgrad_splits(a.K, Cin, Cout, db != nullptr);
  a.Nw = a.N + (db ? 1 : 0);
  a.ldw = (a.Nw + 7) & ~7;
  a.lda = lddy; a.ldb = ldx; a.ldc = a.N;
  a.alpha = 1.0f; a.beta = 0.0f; a.c_f32 = 1;
  a.rps = 1;
  a.colsum = db;
  a.ala = a.alb = 1;
  a.vec_ok = 1;
  a.tiles_m = cdiv(a.M, BM);
  a.tiles_n = cdiv(a.Nw, BN);
  c.H = H; c.W = W; c.Cin = Cin; c.ldx = ldx;
  c.sx = BK % W;
  c.sy = (BK / W) % H;
  auto kern = conv3_igemm_wgrad_kernel<T, BM, BN, NW, WM_, BK>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set = true;
  }
  DFM_LAUNCH(kern, dim3((unsigned)a.tiles_m * a.tiles_n * a.splits), dim3(64 * NW),
             (conv3_lds<T, BM, BN, NW, WM_, BK>(false)), s, c);
  DFM_LAUNCH_CHECK();
  if (a.splits > 1) {
    const long total = (long)a.M * a.ldw;
    if (a.splits >= 8)
      DFM_LAUNCH((conv3_splitk_reduce_kernel<T, 4>), dim3(cdiv(total, 64)), dim3(256), 0, s, a);
    else
      DFM_LAUNCH((conv3_splitk_reduce_kernel<T, 1>), dim3(cdiv(total, 256)), dim3(256), 0, s, a);
    DFM_LAUNCH_CHECK();
  }
  return DFM_OK;
}

bool conv3_shape_ok(int Cin, int Cout) {
  return Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0 && Cin <= 65536 && Cout <= 65536;
}

bool ppm_scales(int s0, int s1, int s2, int s3, PpmScales& sc) {
  const int in[4] = {s0, s1, s2, s3};
  sc.n = 0;
  sc.off[0] = 0;
  for (int k = 0; k < 4; ++k) {
    if (in[k] == 0) break;
    if (in[k] < 0 || in[k] > 16) return false;
    sc.s[sc.n] = in[k];
    sc.off[sc.n + 1] = sc.off[sc.n] + in[k] * in[k];
    ++sc.n;
  }
  for (int k = sc.n; k < 4; ++k) {
    if (in[k] != 0) return false;  // scales are given first, then zeros
    sc.s[k] = 1;
    sc.off[k + 1] = sc.off[k];
  }
  return sc.n > 0;
}

}  // namespace

extern "C" int dfm_conv3s1_igemm_supported(int dtype, int Cin, int Cout) {
  return (dtype == DFM_F32 || dtype == DFM_BF16 || dtype == DFM_F16) && conv3_shape_ok(Cin, Cout) ? 1 : 0;
}

extern "C" int dfm_conv3s1_igemm_fwd(int dtype, int B, int H, int W, int Cin, int Cout, const void* x, long ldx,
                                     const void* wp, const float* bias, void* y, long ldy, int accumulate,
                                     dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(x && wp && y, "dfm_conv3s1_igemm_fwd: null argument");
  DFM_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31) - 256, "dfm_conv3s1_igemm_fwd: bad shape");
  DFM_CHECK_ARG(conv3_shape_ok(Cin, Cout), "dfm_conv3s1_igemm_fwd: Cin=%d, Cout=%d must be multiples of 8", Cin,
                Cout);
  DFM_CHECK_ARG(ldx >= Cin && ldx % 8 == 0 && ldy >= Cout && ldy % 8 == 0,
                "dfm_conv3s1_igemm_fwd: row strides must be multiples of 8 covering Cin / Cout");
  DFM_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)wp % 16 == 0 && (uintptr_t)y % 16 == 0,
                "dfm_conv3s1_igemm_fwd: operands must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  DFM_DTYPE_SWITCH(dtype, T,
                   return conv3_fwd_typed<T>(B, H, W, Cin, Cout, x, ldx, wp, bias, y, ldy, accumulate, s));
}

extern "C" int dfm_conv3_weight_pack_dgrad(int dtype_out, int Cout, int Cin, const float* w, void* wpt,
                                           dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype_out);
  DFM_CHECK_ARG(w && wpt, "dfm_conv3_weight_pack_dgrad: null argument");
  DFM_CHECK_ARG(Cout > 0 && Cin > 0, "dfm_conv3_weight_pack_dgrad: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const long n = 9L * Cout * Cin;
  const unsigned grid = (unsigned)std::min(65536L, (n + 255) / 256);
  DFM_DTYPE_SWITCH(dtype_out, T,
                   DFM_LAUNCH(weight_pack_dgrad_kernel<T>, dim3(grid), dim3(256), 0, s, Cout, Cin, w, (T*)wpt));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" size_t dfm_conv3s1_igemm_wgrad_workspace_size(int dtype, int B, int H, int W, int Cin, int Cout,
                                                         int bias_grad) {
  (void)dtype;
  if (B <= 0 || H <= 0 || W <= 0 || !conv3_shape_ok(Cin, Cout)) return 0;
  const int splits = wgrad_splits((long)B * H * W, Cin, Cout, bias_grad);
  if (splits <= 1) return 0;
  const long ldw = (9L * Cin + (bias_grad ? 1 : 0) + 7) & ~7L;
  return (size_t)splits * Cout * ldw * sizeof(float);
}

extern "C" int dfm_conv3s1_igemm_wgrad(int dtype, int B, int H, int W, int Cin, int Cout, const void* dy, long lddy,
                                       const void* x, long ldx, float* dwp, float* db, void* workspace,
                                       size_t workspace_bytes, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(dy && x && dwp, "dfm_conv3s1_igemm_wgrad: null argument");
  DFM_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31) - 256, "dfm_conv3s1_igemm_wgrad: bad shape");
  DFM_CHECK_ARG(conv3_shape_ok(Cin, Cout), "dfm_conv3s1_igemm_wgrad: Cin=%d, Cout=%d must be multiples of 8", Cin,
                Cout);
  DFM_CHECK_ARG(ldx >= Cin && ldx % 8 == 0 && lddy >= Cout && lddy % 8 == 0,
                "dfm_conv3s1_igemm_wgrad: row strides must be multiples of 8 covering Cin / Cout");
  DFM_CHECK_ARG((uintptr_t)x % 16 == 0 && (uintptr_t)dy % 16 == 0 && (uintptr_t)dwp % 16 == 0,
                "dfm_conv3s1_igemm_wgrad: operands must be 16-byte aligned");
  const size_t need = dfm_conv3s1_igemm_wgrad_workspace_size(dtype, B, H, W, Cin, Cout, db != nullptr);
  DFM_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && (uintptr_t)workspace % 16 == 0),
                "dfm_conv3s1_igemm_wgrad: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0,
                need);
  hipStream_t s = (hipStream_t)stream;
  DFM_DTYPE_SWITCH(dtype, T, return conv3_wgrad_typed<T>(B, H, W, Cin, Cout, dy, lddy, x, ldx, dwp, db, workspace, s));
}

extern "C" int dfm_ppm_pool_fwd(int dtype, int B, int H, int W, int C, int s0, int s1, int s2, int s3, const void* x,
                                long ldx, void* y, long ldy, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(x && y, "dfm_ppm_pool_fwd: null argument");
  DFM_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "dfm_ppm_pool_fwd: C=%d must be a multiple of 8", C);
  PpmScales sc;
  DFM_CHECK_ARG(ppm_scales(s0, s1, s2, s3, sc), "dfm_ppm_pool_fwd: scales must be 1..16, zeros last");
  DFM_CHECK_ARG(ldx >= C && ldx % 8 == 0 && ldy >= C && ldy % 8 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0,
                "dfm_ppm_pool_fwd: operands must be 16-byte aligned with row strides that are multiples of 8");
  DFM_CHECK_ARG((long)B * sc.off[sc.n] < (1L << 30) && (long)H * 16 < (1L << 30) && (long)W * 16 < (1L << 30),
                "dfm_ppm_pool_fwd: shape too large");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * sc.off[sc.n]), cdiv(C / 8, 32));
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(ppm_pool_fwd_kernel<T>, grid, dim3(256), 0, s, B, H, W, C, sc, (const T*)x, ldx, (T*)y, ldy));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_ppm_pool_bwd(int dtype, int B, int H, int W, int C, int s0, int s1, int s2, int s3, const void* dy,
                                long lddy, void* dx, long lddx, int accumulate, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(dy && dx, "dfm_ppm_pool_bwd: null argument");
  DFM_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "dfm_ppm_pool_bwd: C=%d must be a multiple of 8", C);
  PpmScales sc;
  DFM_CHECK_ARG(ppm_scales(s0, s1, s2, s3, sc), "dfm_ppm_pool_bwd: scales must be 1..16, zeros last");
  DFM_CHECK_ARG(lddy >= C && lddy % 8 == 0 && lddx >= C && lddx % 8 == 0 && (uintptr_t)dy % 16 == 0 &&
                    (uintptr_t)dx % 16 == 0,
                "dfm_ppm_pool_bwd: operands must be 16-byte aligned with row strides that are multiples of 8");
  DFM_CHECK_ARG((long)B * sc.off[sc.n] < (1L << 30) && (long)H * 16 < (1L << 30) && (long)W * 16 < (1L << 30),
                "dfm_ppm_pool_bwd: shape too large");
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W * (C / 8);
  const unsigned grid = (unsigned)std::min(65536L, (n + 255) / 256);
  DFM_DTYPE_SWITCH(dtype, T,
                   DFM_LAUNCH(ppm_pool_bwd_kernel<T>, dim3(grid), dim3(256), 0, s, B, H, W, C, sc, (const T*)dy, lddy,
                              (T*)dx, lddx, accumulate));
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
