// Multi-scale + flip evaluation (utils/val_mm.py:325-472 evaluate_msf) and the mIoU confusion
// histogram (utils/metrics_new.py:16-20) on the GPU:
//   dfm_resize_nchw     F.interpolate(img, (Ho, Wo), bilinear, align_corners) [+ torch.flip(dims=3)]
//                       of the rgb / depth inputs, read with any strides (val_mm.py:362-372, 386-388)
//   dfm_msf_accumulate  acc[b, y, x, :] += softmax_c( resize_{align_corners=True}(H, W) of
//                       [flip of] resize_{align_corners=False}(Hs, Ws) of the decoder's low-res
//                       logits )  — the model's own upsampling (builder.py:203), the flip back
//                       (val_mm.py:389) and the resize to the label size (val_mm.py:377-379,
//                       390-392) composed per output pixel: 16 low-res taps, nothing materialised
//   dfm_slide_msf_accumulate  the same with sliding-window inference (val_mm.py:257-322): the scaled
//                       logits are the per-pixel average of the overlapping windows' upsampled
//                       logits, gathered from every window's low-res logits. One kernel serves both:
//                       dfm_msf_accumulate is its case of one window that covers the scaled image
//   dfm_seg_confusion   hist[t * ncls + argmax_c acc[p, c]] += 1 over pixels with t != ignore
// and single-scale evaluation (utils/val_mm.py:102-207 evaluate, 25-98 save_preds):
//   dfm_seg_predict     pred[b, y, x] = argmax_c of the model's own upsampling (builder.py:203) of the
//                       low-res logits, and the confusion histogram of it, in one pass: a workgroup
//                       stages the low-res patch under its rectangle of output pixels in LDS; neither
//                       the full-resolution logits nor their softmax (monotone) exist anywhere
//   dfm_rows_argmax     pred[p] = argmax_c acc[p, c] of score rows (the sliding-window results); the
//                       same kernel as dfm_seg_confusion, which counts the argmax instead of storing it
// Every output element is owned by one thread (no float atomics); the histograms use integer
// atomics, so all of them are deterministic.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxCls = 64;

// PyTorch's source-index rule for bilinear resizing (area_pixel_compute_source_index)
struct Lin {
  int i0, i1;
  float l0, l1;
};
DFM_INLINE Lin lin_src(int dst, int in, int out, bool align) {
  float src;
  if (align) {
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    src = scale * (float)dst;
  } else {
    const float scale = (float)in / (float)out;
    src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  }
  Lin r;
  r.i0 = min((int)src, in - 1);
  r.i1 = min(r.i0 + 1, in - 1);
  r.l1 = src - (float)r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

template <typename Ti, typename To>
__global__ __launch_bounds__(kThreads) void resize_nchw_kernel(int B, int C, int Hi, int Wi, long sb, long sc, long sh,
                                                               long sw, int Ho, int Wo, int align, int flip,
                                                               const Ti* __restrict__ x, To* __restrict__ y) {
  const long n = (long)B * C * Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % Wo);
    long t = i / Wo;
    const int oy = (int)(t % Ho);
    t /= Ho;
    const int c = (int)(t % C);
    const long b = t / C;
    const Lin ly = lin_src(oy, Hi, Ho, align), lx = lin_src(flip ? Wo - 1 - ox : ox, Wi, Wo, align);
    const Ti* p = x + b * sb + c * sc;
    const float v = ly.l0 * (lx.l0 * ldf(p + ly.i0 * sh + lx.i0 * sw) + lx.l1 * ldf(p + ly.i0 * sh + lx.i1 * sw)) +
                    ly.l1 * (lx.l0 * ldf(p + ly.i1 * sh + lx.i0 * sw) + lx.l1 * ldf(p + ly.i1 * sh + lx.i1 * sw));
    stf(y + i, v);
  }
}

// The accumulate kernel, in its sliding-window form (val_mm.py:257-322 slide_inference inside
// evaluate_msf): the scaled image is covered by hg x wg windows of hc x wc pixels, window (gi, gj)
// starting at (win_start(gi, hstride, hc, Hs), win_start(gj, wstride, wc, Ws)); low holds every window's
// low-res logits, [hg*wg][B][h][w] rows. Per output pixel the 4 align_corners=True taps of the scaled
// grid are each the average over the covering windows (ascending (gi, gj), summed then divided by the
// count, like the reference's preds / count_mat) of that window's align_corners=False upsampling at the
// tap: nothing of size [B, ncls, Hs, Ws] is materialised. Plain multi-scale evaluation
// (dfm_msf_accumulate) is its one-window case: crop = stride = (Hs, Ws), hg = wg = 1, count 1.
DFM_INLINE int win_start(int g, int stride, int crop, int n) { return max(min(g * stride + crop, n) - crop, 0); }

// kSlideLanes lanes share an output pixel: lane j owns classes j, j + kSlideLanes, ..., so a group's
// loads of a low-res tap and its read-modify-write of the pixel's acc row are contiguous across lanes
// (one thread per pixel strides ncls floats between lanes: measured 2.3-2.8x slower); the
// softmax's max and sum go across the group's lanes.
constexpr int kSlideLanes = 8;
template <int G> DFM_INLINE float group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename T, int KC>
__global__ __launch_bounds__(kThreads) void slide_msf_accumulate_kernel(
    int B, int h, int w, int ncls, const T* __restrict__ low, long ldl, int hc, int wc, int hstride, int wstride,
    int hg, int wg, int Hs, int Ws, int H, int W, int flip, int softmax, float* __restrict__ acc) {
  constexpr int L = kSlideLanes, kPix = kThreads / L;
  const int j = threadIdx.x % L;
  const long n = (long)B * H * W;
  // a group's lanes share p, so they leave the loop together and the cross-lane steps stay inside it
  for (long p = blockIdx.x * (long)kPix + threadIdx.x / L; p < n; p += (long)gridDim.x * kPix) {
    const int x = (int)(p % W);
    const long t = p / W;
    const int y = (int)(t % H);
    const long b = t / H;
    float z[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) z[k] = 0.f;
    const Lin sy = lin_src(y, Hs, H, true), sx = lin_src(x, Ws, W, true);
    for (int a = 0; a < 4; ++a) {
      const int ys = (a >> 1) ? sy.i1 : sy.i0;
      const int xs0 = (a & 1) ? sx.i1 : sx.i0;
      const float wa = ((a >> 1) ? sy.l1 : sy.l0) * ((a & 1) ? sx.l1 : sx.l0);
      const int xs = flip ? Ws - 1 - xs0 : xs0;
      float l[KC];
#pragma unroll
      for (int k = 0; k < KC; ++k) l[k] = 0.f;
      int count = 0;
      for (int gi = 0; gi < hg; ++gi) {
        const int y1 = win_start(gi, hstride, hc, Hs);
        if (ys < y1 || ys >= y1 + hc) continue;
        const Lin ly = lin_src(ys - y1, h, hc, false);
        for (int gj = 0; gj < wg; ++gj) {
          const int x1 = win_start(gj, wstride, wc, Ws);
          if (xs < x1 || xs >= x1 + wc) continue;
          const Lin lx = lin_src(xs - x1, w, wc, false);
          const T* img = low + (((long)(gi * wg + gj) * B + b) * h) * w * ldl + j;
          const T* p00 = img + ((long)ly.i0 * w + lx.i0) * ldl;
          const T* p01 = img + ((long)ly.i0 * w + lx.i1) * ldl;
          const T* p10 = img + ((long)ly.i1 * w + lx.i0) * ldl;
          const T* p11 = img + ((long)ly.i1 * w + lx.i1) * ldl;
#pragma unroll
          for (int k = 0; k < KC; ++k)
            if (j + k * L < ncls)
              l[k] += ly.l0 * (lx.l0 * ldf(p00 + k * L) + lx.l1 * ldf(p01 + k * L)) +
                      ly.l1 * (lx.l0 * ldf(p10 + k * L) + lx.l1 * ldf(p11 + k * L));
          ++count;
        }
      }
      const float cnt = (float)count;
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (j + k * L < ncls) z[k] = fmaf(wa, l[k] / cnt, z[k]);
    }
    float* dst = acc + p * ncls + j;
    if (!softmax) {
#pragma unroll
      for (int k = 0; k < KC; ++k)
        if (j + k * L < ncls) dst[k * L] = z[k];
      continue;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (j + k * L < ncls) mx = fmaxf(mx, z[k]);
    mx = group_max<L>(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (j + k * L < ncls) {
        z[k] = expf(z[k] - mx);
        s += z[k];
      }
    const float inv = 1.f / group_sum<L>(s);
#pragma unroll
    for (int k = 0; k < KC; ++k)
      if (j + k * L < ncls) dst[k * L] += z[k] * inv;
  }
}

// ---- dfm_seg_predict. A workgroup owns kPredTY x kPredTX output pixels of one image; thread t owns
// the 4 consecutive pixels x0 + 4 * (t % 16) ... of row y0 + t / 16 (its uint8 predictions are one
// dword). The low-res cells those pixels interpolate from are a rectangle: rows lin_src(first y).i0 ..
// lin_src(last y).i1, columns likewise (the source index is monotone in the destination), whatever the
// factor. It is staged once, converted to fp32, as patch[cell][cs] with the classes of a cell contiguous
// and a padded class stride cs = 4 * odd: a tap's 4 consecutive classes are one 16-byte LDS read, the
// lanes of a read group sit on neighbouring cells, whose 16-byte slots differ (cs / 4 odd; lanes under
// the same cell broadcast), and the staging writes of a cell's classes are consecutive. When the patch
// times ncls exceeds the LDS budget (small factors: the identity needs 17 x 65 cells) the classes go
// through in chunks of cs; the running (value, class) pair keeps the first maximum across chunks, so
// nothing per class lives in registers and one instantiation per dtype serves every ncls.
constexpr int kPredTX = 64, kPredTY = 16;
constexpr int kPredPatchFloats = 8192;  // 32 KiB of patch + at most 16 KiB of histogram per workgroup
constexpr int kPredMaxBlocks = 1536;    // about what one MI355X holds at a time (6 workgroups x 256 CUs)
static_assert(kPredTX / 4 * kPredTY == kThreads, "one thread per 4 pixels of the rectangle");

template <typename T>
__global__ __launch_bounds__(kThreads) void seg_predict_kernel(int h, int w, int ncls, const T* __restrict__ low,
                                                               long ldl, int H, int W, int tiles_x, int tiles_y,
                                                               long ntiles, int cs, int cap, int vec,
                                                               unsigned char* __restrict__ pred,
                                                               const long long* __restrict__ label, int ignore,
                                                               unsigned long long* __restrict__ hist) {
  // cap floats of patch, then ncls * ncls counters when there is a label
  extern __shared__ __attribute__((aligned(16))) float patch[];
  unsigned int* lh = reinterpret_cast<unsigned int*>(patch + cap);
  const float4_t* patch4 = reinterpret_cast<const float4_t*>(patch);
  const int tid = threadIdx.x, cs4 = cs / 4;
  if (label)
    for (int i = tid; i < ncls * ncls; i += kThreads) lh[i] = 0u;
  // with a label a workgroup takes several rectangles (neighbouring workgroups neighbouring ones) and
  // flushes its counters once: fewer global atomics on the ncls * ncls bins
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int x0 = (int)(tile % tiles_x) * kPredTX, y0 = (int)(tile / tiles_x % tiles_y) * kPredTY;
    const long b = tile / ((long)tiles_x * tiles_y);
    const int xe = min(x0 + kPredTX, W) - 1, ye = min(y0 + kPredTY, H) - 1;  // the rectangle's last pixel
    const int ry0 = lin_src(y0, h, H, false).i0, rx0 = lin_src(x0, w, W, false).i0;
    const int ph = lin_src(ye, h, H, false).i1 - ry0 + 1, pw = lin_src(xe, w, W, false).i1 - rx0 + 1;
    const int cells = ph * pw;
    if (cells * cs > cap) break;  // never: the entry point sizes cap for the largest patch of this geometry

    const int xb = x0 + 4 * (tid % (kPredTX / 4)), y = y0 + tid / (kPredTX / 4);
    // pixels beyond the image compute the last pixel's value (inside the patch) and store nothing
    const Lin ly = lin_src(min(y, ye), h, H, false);
    const int r0 = (ly.i0 - ry0) * pw, r1 = (ly.i1 - ry0) * pw;
    int f00[4], f01[4], f10[4], f11[4], best[4];  // the four taps' cells, as 16-byte offsets into the patch
    float a0[4], a1[4], bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const Lin lx = lin_src(min(xb + i, xe), w, W, false);
      f00[i] = (r0 + lx.i0 - rx0) * cs4;
      f01[i] = (r0 + lx.i1 - rx0) * cs4;
      f10[i] = (r1 + lx.i0 - rx0) * cs4;
      f11[i] = (r1 + lx.i1 - rx0) * cs4;
      a0[i] = lx.l0;
      a1[i] = lx.l1;
      best[i] = 0;
      bv[i] = -INFINITY;
    }
    const T* src = low + ((b * h + ry0) * w + rx0) * ldl;
    for (int c0 = 0; c0 < ncls; c0 += cs) {
      const int nc = min(cs, ncls - c0);
      __syncthreads();  // the previous chunk, or rectangle, has been read
      for (int i = tid; i < cells * nc; i += kThreads) {  // consecutive lanes: consecutive classes of a cell
        const int cc = i % nc, cell = i / nc;
        const int px = cell % pw, py = cell / pw;
        patch[cell * cs + cc] = ldf(src + ((long)py * w + px) * ldl + c0 + cc);
      }
      __syncthreads();
      for (int cc = 0; cc < nc; cc += 4) {  // the columns from nc up to the next multiple of 4 are never staged
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4_t t00 = patch4[f00[i] + cc / 4], t01 = patch4[f01[i] + cc / 4];
          const float4_t t10 = patch4[f10[i] + cc / 4], t11 = patch4[f11[i] + cc / 4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float v = ly.l0 * (a0[i] * t00[k] + a1[i] * t01[k]) + ly.l1 * (a0[i] * t10[k] + a1[i] * t11[k]);
            if (cc + k < nc && v > bv[i]) {  // first maximum wins, like torch.argmax
              bv[i] = v;
              best[i] = c0 + cc + k;
            }
          }
        }
      }
    }

    if (y < H) {
      const long row = (b * H + y) * W;
      if (label) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (xb + i >= W) continue;
          const long long t = label[row + xb + i];
          if (t == ignore || t < 0 || t >= ncls) continue;
          atomicAdd(&lh[t * ncls + best[i]], 1u);
        }
      }
      if (pred) {
        if (vec && xb + 3 < W) {
          *reinterpret_cast<unsigned int*>(pred + row + xb) =
              (unsigned)best[0] | (unsigned)best[1] << 8 | (unsigned)best[2] << 16 | (unsigned)best[3] << 24;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (xb + i < W) pred[row + xb + i] = (unsigned char)best[i];
        }
      }
    }
  }
  if (label) {
    __syncthreads();
    for (int i = tid; i < ncls * ncls; i += kThreads)
      if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
  }
}

// The row argmax of dfm_rows_argmax (pred) and dfm_seg_confusion (label, ignore, hist; ncls * ncls
// counters of LDS): kSlideLanes lanes share a row of scores (contiguous loads); the group's (value, class)
// pairs reduce to the first maximum, which lane 0 stores and / or counts into the workgroup's histogram;
// the workgroup flushes its counters once.
__global__ __launch_bounds__(kThreads) void rows_argmax_kernel(long npix, int ncls, const float* __restrict__ acc,
                                                               unsigned char* __restrict__ pred,
                                                               const long long* __restrict__ label, int ignore,
                                                               unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned int lh[];
  constexpr int L = kSlideLanes, kPix = kThreads / L;
  const int j = threadIdx.x % L;
  if (label) {
    for (int i = threadIdx.x; i < ncls * ncls; i += kThreads) lh[i] = 0u;
    __syncthreads();
  }
  // a group's lanes share p, so they leave the loop together and the cross-lane steps stay inside it
  for (long p = blockIdx.x * (long)kPix + threadIdx.x / L; p < npix; p += (long)gridDim.x * kPix) {
    const float* a = acc + p * ncls;
    float bv = -INFINITY;
    int best = kMaxCls;  // a lane without a class loses every tie
    if (j < ncls) {
      bv = a[j];
      best = j;
    }
    for (int c = j + L; c < ncls; c += L) {
      const float v = a[c];
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int ob = __shfl_xor(best, o, 64);
      if (ov > bv || (ov == bv && ob < best)) {
        bv = ov;
        best = ob;
      }
    }
    if (j != 0) continue;
    if (pred) pred[p] = (unsigned char)best;
    if (label) {
      const long long t = label[p];
      if (t != ignore && t >= 0 && t < ncls) atomicAdd(&lh[t * ncls + best], 1u);
    }
  }
  if (label) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncls * ncls; i += kThreads)
      if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
  }
}

unsigned grid_for(long n, long cap = 16384) {
  const long g = (n + kThreads - 1) / kThreads;
  return (unsigned)(g < cap ? (g < 1 ? 1 : g) : cap);
}

int slide_grids(int n, int crop, int stride) {  // val_mm.py:295-296
  const int over = n - crop + stride - 1;
  return (over > 0 ? over : 0) / stride + 1;
}

template <typename T>
int slide_msf_typed(int B, int h, int w, int ncls, const void* low, long ldl, int hc, int wc, int hstride, int wstride,
                    int Hs, int Ws, int H, int W, int flip, int softmax, float* acc, hipStream_t s) {
  const int hg = slide_grids(Hs, hc, hstride), wg = slide_grids(Ws, wc, wstride);
  const unsigned g = grid_for((long)B * H * W * kSlideLanes);
#define DFM_SLIDE(NC)                                                                                        \
  DFM_LAUNCH((slide_msf_accumulate_kernel<T, NC / kSlideLanes>), dim3(g), dim3(kThreads), 0, s, B, h, w, ncls, \
             (const T*)low, ldl, hc, wc, hstride, wstride, hg, wg, Hs, Ws, H, W, flip, softmax, acc)
  if (ncls <= 16) DFM_SLIDE(16);
  else if (ncls <= 40) DFM_SLIDE(40);
  else DFM_SLIDE(kMaxCls);
#undef DFM_SLIDE
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

template <typename T>
int seg_predict_typed(int B, int h, int w, int ncls, const void* low, long ldl, int H, int W, unsigned char* pred,
                      const long long* label, int ignore, unsigned long long* hist, hipStream_t s) {
  // the most rows / columns a rectangle's patch can span: the source index moves by at most
  // ceil((n - 1) * in / out) over n pixels, + 1 for the second tap, + 1 for fp32 rounding of the index
  const int phb = (int)std::min<long>(h, ((long)(kPredTY - 1) * h + H - 1) / H + 3);
  const int pwb = (int)std::min<long>(w, ((long)(kPredTX - 1) * w + W - 1) / W + 3);
  const int cells = phb * pwb;  // <= 18 * 66: four classes of every cell always fit
  // the class stride in units of 4 floats, odd: all of ncls when that fits the budget, else a chunk
  const int q_all = (int)cdiv(ncls, 4) | 1, q_fit = kPredPatchFloats / (4 * cells);
  const int cs = 4 * (q_all <= q_fit ? q_all : (q_fit - 1) | 1);
  const int cap = cells * cs;
  const size_t lds = (size_t)cap * sizeof(float) + (label ? (size_t)ncls * ncls * sizeof(unsigned int) : 0);
  const int vec = pred && W % 4 == 0 && (uintptr_t)pred % 4 == 0;  // a thread's 4 predictions as one dword
  const int tiles_x = (int)cdiv(W, kPredTX), tiles_y = (int)cdiv(H, kPredTY);
  const long ntiles = (long)B * tiles_y * tiles_x;
  // rectangles per workgroup, the same for all: one without a label (the most workgroups to overlap staging
  // and arithmetic: measured 75 vs 96 us at 16 x 480 x 640), else as many as keep the chip full once
  // (a quarter of the counter flushes there: 105 vs 128 us with the label)
  const long per = label ? (ntiles + kPredMaxBlocks - 1) / kPredMaxBlocks : 1;
  DFM_LAUNCH((seg_predict_kernel<T>), dim3(cdiv(ntiles, per)), dim3(kThreads), lds, s, h, w, ncls, (const T*)low, ldl,
             H, W, tiles_x, tiles_y, ntiles, cs, cap, vec, pred, label, ignore, hist);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

}  // namespace

extern "C" int dfm_resize_nchw(int dtype_in, int dtype_out, int B, int C, int Hi, int Wi, long sb, long sc, long sh,
                               long sw, const void* x, int Ho, int Wo, int align_corners, int flip, void* y,
                               dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype_in);
  DFM_CHECK_DTYPE(dtype_out);
  DFM_CHECK_ARG(x && y && B > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "dfm_resize_nchw: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = grid_for((long)B * C * Ho * Wo);
#define DFM_RESIZE(TI, TO)                                                                                          \
  DFM_LAUNCH((resize_nchw_kernel<TI, TO>), dim3(g), dim3(kThreads), 0, s, B, C, Hi, Wi, sb, sc, sh, sw, Ho, Wo,      \
             align_corners, flip, (const TI*)x, (TO*)y)
  // the instantiated (in, out) pairs, as an explicit table
  if (dtype_in == DFM_F32 && dtype_out == DFM_F32) DFM_RESIZE(float, float);
  else if (dtype_in == DFM_BF16 && dtype_out == DFM_F32) DFM_RESIZE(bf16_t, float);
  else if (dtype_in == DFM_F32 && dtype_out == DFM_BF16) DFM_RESIZE(float, bf16_t);
  else if (dtype_in == DFM_BF16 && dtype_out == DFM_BF16) DFM_RESIZE(bf16_t, bf16_t);
  else if (dtype_in == DFM_F16 && dtype_out == DFM_F32) DFM_RESIZE(f16_t, float);
  else if (dtype_in == DFM_F32 && dtype_out == DFM_F16) DFM_RESIZE(float, f16_t);
  else {
    dfm_set_error("dfm_resize_nchw: unsupported dtype %d -> %d", dtype_in, dtype_out);
    return DFM_ERR_DTYPE;
  }
#undef DFM_RESIZE
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_msf_accumulate(int dtype, int B, int h, int w, int ncls, const void* low, long ldl, int Hs, int Ws,
                                  int H, int W, int flip, float* acc, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(low && acc && B > 0 && h > 0 && w > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && ldl >= ncls,
                "dfm_msf_accumulate: bad argument");
  DFM_CHECK_ARG(ncls > 0 && ncls <= kMaxCls, "dfm_msf_accumulate: ncls=%d outside [1, %d]", ncls, kMaxCls);
  hipStream_t s = (hipStream_t)stream;
  // one window that covers the scaled image
  DFM_DTYPE_SWITCH(dtype, T,
                   return slide_msf_typed<T>(B, h, w, ncls, low, ldl, Hs, Ws, Hs, Ws, Hs, Ws, H, W, flip, 1, acc, s));
}

extern "C" int dfm_slide_msf_accumulate(int dtype, int B, int h, int w, int ncls, const void* low, long ldl, int hc,
                                        int wc, int hstride, int wstride, int Hs, int Ws, int H, int W, int flip,
                                        int softmax, float* acc, dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(low && acc, "dfm_slide_msf_accumulate: null pointer");
  DFM_CHECK_ARG(ncls > 0 && ncls <= kMaxCls, "dfm_slide_msf_accumulate: ncls=%d outside [1, %d]", ncls, kMaxCls);
  DFM_CHECK_ARG(B > 0 && h > 0 && w > 0 && hc > 0 && wc > 0 && H > 0 && W > 0 && ldl >= ncls,
                "dfm_slide_msf_accumulate: bad argument");
  DFM_CHECK_ARG(hstride > 0 && wstride > 0, "dfm_slide_msf_accumulate: stride %d x %d must be positive", hstride,
                wstride);
  // a stride beyond the crop would leave pixels that no window covers (the reference asserts on them)
  DFM_CHECK_ARG(hstride <= hc && wstride <= wc, "dfm_slide_msf_accumulate: stride %d x %d exceeds the crop %d x %d",
                hstride, wstride, hc, wc);
  DFM_CHECK_ARG(Hs >= hc && Ws >= wc, "dfm_slide_msf_accumulate: scaled size %d x %d smaller than the crop %d x %d",
                Hs, Ws, hc, wc);
  hipStream_t s = (hipStream_t)stream;
  DFM_DTYPE_SWITCH(dtype, T, return slide_msf_typed<T>(B, h, w, ncls, low, ldl, hc, wc, hstride, wstride, Hs, Ws, H, W,
                                                       flip, softmax, acc, s));
}

extern "C" int dfm_seg_confusion(long npix, int ncls, const float* acc, const long long* label, int ignore,
                                 unsigned long long* hist, dfm_stream_t stream) {
  DFM_CHECK_ARG(acc && label && hist && npix >= 0 && ncls > 0 && ncls <= kMaxCls,
                "dfm_seg_confusion: bad argument (ncls <= %d)", kMaxCls);
  if (npix == 0) return DFM_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)ncls * ncls * sizeof(unsigned int);
  // a smaller grid than dfm_rows_argmax's: every workgroup flushes ncls * ncls counters
  DFM_LAUNCH(rows_argmax_kernel, dim3(grid_for(npix * kSlideLanes, 2048)), dim3(kThreads), lds, s, npix, ncls, acc,
             (unsigned char*)nullptr, label, ignore, hist);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_seg_predict(int dtype, int B, int h, int w, int ncls, const void* low, long ldl, int H, int W,
                               unsigned char* pred, const long long* label, int ignore, unsigned long long* hist,
                               dfm_stream_t stream) {
  DFM_CHECK_DTYPE(dtype);
  DFM_CHECK_ARG(low, "dfm_seg_predict: null pointer (low)");
  DFM_CHECK_ARG(ncls > 0 && ncls <= kMaxCls, "dfm_seg_predict: ncls=%d outside [1, %d]", ncls, kMaxCls);
  DFM_CHECK_ARG(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && ldl >= ncls,
                "dfm_seg_predict: bad argument");
  DFM_CHECK_ARG(h <= H && w <= W, "dfm_seg_predict: low-res size %d x %d exceeds the output %d x %d (upsampling only)",
                h, w, H, W);
  DFM_CHECK_ARG(pred || hist || label, "dfm_seg_predict: no output (pred and hist are both null)");
  DFM_CHECK_ARG((label != nullptr) == (hist != nullptr), "dfm_seg_predict: label and hist go together");
  hipStream_t s = (hipStream_t)stream;
  DFM_DTYPE_SWITCH(dtype, T, return seg_predict_typed<T>(B, h, w, ncls, low, ldl, H, W, pred, label, ignore, hist, s));
}

extern "C" int dfm_rows_argmax(long npix, int ncls, const float* acc, unsigned char* pred, dfm_stream_t stream) {
  DFM_CHECK_ARG(acc && pred, "dfm_rows_argmax: null pointer");
  DFM_CHECK_ARG(ncls > 0 && ncls <= kMaxCls, "dfm_rows_argmax: ncls=%d outside [1, %d]", ncls, kMaxCls);
  DFM_CHECK_ARG(npix >= 0, "dfm_rows_argmax: bad argument");
  if (npix == 0) return DFM_OK;
  hipStream_t s = (hipStream_t)stream;
  DFM_LAUNCH(rows_argmax_kernel, dim3(grid_for(npix * kSlideLanes)), dim3(kThreads), 0, s, npix, ncls, acc, pred,
             (const long long*)nullptr, 0, (unsigned long long*)nullptr);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
