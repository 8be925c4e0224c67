// libdformer_data.so: the loader's TrainPre (mirror, resize, normalise, crop, pad) for a batch of raw uint8
// images as one kernel (include/dformer_data.h states the semantics). Bandwidth-shaped: one thread
// writes 4 consecutive output x of one row of every plane (16-byte stores for the float planes, 2 x 16
// bytes for the int64 label); the sources are gathered bytes of a few MB that stay in L2. The
// per-sample parameters are read at a block-uniform address, so they travel as scalar loads.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../../include/dformer_data.h"

static thread_local char g_err[256] = "";

static void dfd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* dfd_last_error(void) { return g_err; }
extern "C" int dfd_abi_version(void) { return 1; }

#define DFD_CHECK_ARG(cond, ...)  \
  do {                            \
    if (!(cond)) {                \
      dfd_set_error(__VA_ARGS__); \
      return DFD_ERR_ARG;         \
    }                             \
  } while (0)

namespace {

typedef __attribute__((ext_vector_type(2))) long long ll2_t;

struct PreArgs {
  const uint8_t* rgb;
  const uint8_t* modal;
  const uint8_t* gt;
  const int* params;
  float* out_rgb;
  float* out_modal;
  long long* out_label;
  int H0, W0, ch, cw;
  int ngx;  // groups of 4 output x per row
  int bgr, transform_gt;
  int vec;  // cw % 4 == 0 and 16-byte aligned outputs: vector stores
  float mean[3], std[3], mmean[3], mstd[3];
};

struct Tap {
  int s0, s1;
  float w;
};

// Half-pixel bilinear taps of index r of an axis scaled from n0 to ns samples (1 <= ns <= DFD_MAX_SCALED,
// n0 <= DFD_MAX_DIM, r < ns: every product below stays under 2^30). Exact integers, so the weight is the
// correctly rounded quotient.
__device__ __forceinline__ Tap lin_tap(int r, int n0, int ns) {
  if (r < 0) return Tap{0, 0, 0.f};
  const int num = (2 * r + 1) * n0 - ns;
  if (num < 0) return Tap{0, 0, 0.f};
  const unsigned den = 2u * (unsigned)ns;
  const unsigned s0 = (unsigned)num / den;
  if (s0 >= (unsigned)(n0 - 1)) return Tap{n0 - 1, n0 - 1, 0.f};
  return Tap{(int)s0, (int)s0 + 1, (float)((unsigned)num - s0 * den) / (float)den};
}

// cv2.INTER_NEAREST's source index of r, clamped to the axis
__device__ __forceinline__ int near_tap(int r, int n0, int ns) {
  if (r < 0) return 0;
  return min((int)((unsigned)(r * n0) / (unsigned)ns), n0 - 1);
}

// the part [0, lim] of n - pos, with pos unchecked device data
__device__ __forceinline__ int crop_extent(int n, int pos, int lim) {
  const long long d = (long long)n - pos;
  return d <= 0 ? 0 : (d >= lim ? lim : (int)d);
}

// position in the scaled image of crop offset o >= 0 (below the scaled size by crop_extent); any
// negative value stands for "before the image"
__device__ __forceinline__ int scaled_pos(int pos, int o) {
  const long long r = (long long)pos + o;
  return r < 0 ? -1 : (int)r;
}

template <int CM>
__global__ __launch_bounds__(256) void train_pre_kernel(PreArgs a) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= a.ch * a.ngx) return;
  const int b = blockIdx.y;
  const int y = g / a.ngx, x0 = (g - y * a.ngx) * 4;

  const int* p = a.params + (size_t)b * 8;
  const bool flip = p[0] != 0;
  const int sh = p[1], sw = p[2], pos_h = p[3], pos_w = p[4];
  const bool live = sh > 0 && sw > 0 && sh <= DFD_MAX_SCALED && sw <= DFD_MAX_SCALED;
  const int hc = live ? crop_extent(sh, pos_h, a.ch) : 0;
  const int wc = live ? crop_extent(sw, pos_w, a.cw) : 0;
  const int yy = y - (a.ch - hc) / 2;
  const int pl = (a.cw - wc) / 2;
  const bool interp = sh != a.H0 || sw != a.W0;  // the unscaled image needs one tap: every weight is 0

  float o_rgb[3][4], o_mod[CM][4];
  long long o_lab[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o_rgb[c][j] = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) o_mod[c][j] = 0.f;
    o_lab[j] = 255;
  }

  if (yy >= 0 && yy < hc) {
    const int r = scaled_pos(pos_h, yy);
    const Tap ty = lin_tap(r, a.H0, sh);
    const size_t img = (size_t)b * a.H0;
    const size_t row0 = (img + ty.s0) * a.W0, row1 = (img + ty.s1) * a.W0;
    const size_t rowl = (img + near_tap(r, a.H0, sh)) * a.W0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = x0 + j - pl;
      if (xx < 0 || xx >= wc) continue;  // also every x >= cw of the last group: pl + wc <= cw
      const int c = scaled_pos(pos_w, xx);
      const Tap tx = lin_tap(c, a.W0, sw);
      const int c0 = flip ? a.W0 - 1 - tx.s0 : tx.s0, c1 = flip ? a.W0 - 1 - tx.s1 : tx.s1;
      const size_t i00 = row0 + c0, i01 = row0 + c1, i10 = row1 + c0, i11 = row1 + c1;
      auto sample = [&](const uint8_t* src, int nch, int sc) -> float {
        const float v00 = (float)src[i00 * nch + sc];
        if (!interp) return v00;
        const float v01 = (float)src[i01 * nch + sc], v10 = (float)src[i10 * nch + sc];
        const float v11 = (float)src[i11 * nch + sc];
        const float top = fmaf(tx.w, v01 - v00, v00), bot = fmaf(tx.w, v11 - v10, v10);
        return floorf(fmaf(ty.w, bot - top, top) + 0.5f);
      };
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o_rgb[k][j] = (sample(a.rgb, 3, a.bgr ? 2 - k : k) / 255.0f - a.mean[k]) / a.std[k];
#pragma unroll
      for (int k = 0; k < CM; ++k)
        o_mod[k][j] = (sample(a.modal, CM, CM == 3 && a.bgr ? 2 - k : k) / 255.0f - a.mmean[k]) / a.mstd[k];
      const int cl = near_tap(c, a.W0, sw);
      const int gv = a.gt[rowl + (flip ? a.W0 - 1 - cl : cl)];
      o_lab[j] = a.transform_gt ? ((gv - 1) & 255) : gv;
    }
  }

  const size_t plane = (size_t)a.ch * a.cw, at = (size_t)y * a.cw + x0;
  float* d_rgb = a.out_rgb + (size_t)b * 3 * plane + at;
  float* d_mod = a.out_modal + (size_t)b * CM * plane + at;
  long long* d_lab = a.out_label + (size_t)b * plane + at;
  if (a.vec) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      *reinterpret_cast<float4*>(d_rgb + k * plane) = make_float4(o_rgb[k][0], o_rgb[k][1], o_rgb[k][2], o_rgb[k][3]);
#pragma unroll
    for (int k = 0; k < CM; ++k)
      *reinterpret_cast<float4*>(d_mod + k * plane) = make_float4(o_mod[k][0], o_mod[k][1], o_mod[k][2], o_mod[k][3]);
    reinterpret_cast<ll2_t*>(d_lab)[0] = ll2_t{o_lab[0], o_lab[1]};
    reinterpret_cast<ll2_t*>(d_lab)[1] = ll2_t{o_lab[2], o_lab[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j >= a.cw) break;
#pragma unroll
      for (int k = 0; k < 3; ++k) d_rgb[k * plane + j] = o_rgb[k][j];
#pragma unroll
      for (int k = 0; k < CM; ++k) d_mod[k * plane + j] = o_mod[k][j];
      d_lab[j] = o_lab[j];
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int dfd_train_pre(const DfdPreDesc* d, const void* rgb, const void* modal, const void* gt,
                             const void* params, void* out_rgb, void* out_modal, void* out_label,
                             dfd_stream_t stream) {
  DFD_CHECK_ARG(d && rgb && modal && gt && params && out_rgb && out_modal && out_label,
                "dfd_train_pre: null descriptor or pointer");
  DFD_CHECK_ARG(d->B > 0 && d->B <= 65535, "dfd_train_pre: batch %d outside 1..65535", d->B);
  DFD_CHECK_ARG(d->H0 > 0 && d->W0 > 0 && d->H0 <= DFD_MAX_DIM && d->W0 <= DFD_MAX_DIM,
                "dfd_train_pre: raw size %d x %d outside 1..%d", d->H0, d->W0, DFD_MAX_DIM);
  DFD_CHECK_ARG(d->ch > 0 && d->cw > 0 && d->ch <= DFD_MAX_DIM && d->cw <= DFD_MAX_DIM,
                "dfd_train_pre: crop size %d x %d outside 1..%d", d->ch, d->cw, DFD_MAX_DIM);
  DFD_CHECK_ARG(d->modal_channels == 1 || d->modal_channels == 3, "dfd_train_pre: modal_channels %d, want 1 or 3",
                d->modal_channels);
  for (int k = 0; k < 3; ++k)
    DFD_CHECK_ARG(d->std[k] > 0.f && d->modal_std[k] > 0.f, "dfd_train_pre: std[%d] must be > 0", k);

  PreArgs a;
  a.rgb = (const uint8_t*)rgb;
  a.modal = (const uint8_t*)modal;
  a.gt = (const uint8_t*)gt;
  a.params = (const int*)params;
  a.out_rgb = (float*)out_rgb;
  a.out_modal = (float*)out_modal;
  a.out_label = (long long*)out_label;
  a.H0 = d->H0, a.W0 = d->W0, a.ch = d->ch, a.cw = d->cw;
  a.ngx = (d->cw + 3) / 4;
  a.bgr = d->bgr != 0, a.transform_gt = d->transform_gt != 0;
  a.vec = d->cw % 4 == 0 && aligned16(out_rgb) && aligned16(out_modal) && aligned16(out_label);
  for (int k = 0; k < 3; ++k) {
    a.mean[k] = d->mean[k], a.std[k] = d->std[k];
    a.mmean[k] = d->modal_mean[k], a.mstd[k] = d->modal_std[k];
  }
  const dim3 grid((unsigned)(((long)d->ch * a.ngx + 255) / 256), (unsigned)d->B);
  if (d->modal_channels == 1) hipLaunchKernelGGL(train_pre_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(train_pre_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    dfd_set_error("dfd_train_pre: launch failed: %s", hipGetErrorString(e));
    return DFD_ERR_LAUNCH;
  }
  return DFD_OK;
}
