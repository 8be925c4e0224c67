// The optimizer tail of a training step over the flat float32 group buffers: the AdamW update, the
// fp16 loss scaler, and FusedAdamW's options (gradient accumulation, clipping by the global gradient
// norm, an exponential moving average of the weights).
// Every decision a step takes (is this the window's last micro-step, did the fp16 gradients
// overflow, how much to clip) is read from device memory, so one captured HIP graph serves every
// micro-step. Reductions are two-stage with a fixed order: no float atomics, bit-reproducible.
#include <algorithm>

#include "common.h"

namespace {
constexpr int SUMSQ_BLOCKS = 1024;  // stage-one grid of the sum of squares: one partial per block, any n

// win = {micro_index, accum_steps} (int32, NULL = no window): true on every micro-step of an
// accumulation window but its last, where the window's kernels have nothing to do yet
DFM_INLINE bool window_open(const int* __restrict__ win) { return win && win[0] != win[1] - 1; }

unsigned opt_grid(long n) { return (unsigned)std::min((long)8192, std::max(1L, (n + 255) / 256)); }
bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

// acc += g. n4 float4 pairs (16-byte aligned buffers), then the scalar tail.
__global__ void grad_accumulate_kernel(long n, long n4, float* __restrict__ acc, const float* __restrict__ g) {
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long i = t; i < n4; i += stride) {
    float4 a = reinterpret_cast<float4*>(acc)[i];
    const float4 b = reinterpret_cast<const float4*>(g)[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(acc)[i] = a;
  }
  for (long i = 4 * n4 + t; i < n; i += stride) acc[i] += g[i];
}

// Stage one of sum g[i]^2: SUMSQ_BLOCKS blocks, part[block] = the block's share (grid-stride, four
// accumulators per thread, wave butterfly, the four waves in order). With `flag`, also the
// GradScaler's found_inf over the same read (flag[0] = 1 if any element is inf / nan).
__global__ __launch_bounds__(256) void grad_sumsq_kernel(long n, long n4, const float* __restrict__ g,
                                                         float* __restrict__ part, int* __restrict__ flag,
                                                         const int* __restrict__ win) {
  if (window_open(win)) return;
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  bool bad = false;
  for (long i = t; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(g)[i];
    s0 += a.x * a.x; s1 += a.y * a.y; s2 += a.z * a.z; s3 += a.w * a.w;
    bad |= !(isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(a.w));
  }
  for (long i = 4 * n4 + t; i < n; i += stride) {
    s0 += g[i] * g[i];
    bad |= !isfinite(g[i]);
  }
  const float s = wave_sum((s0 + s1) + (s2 + s3));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  if (flag && __any(bad) && (threadIdx.x & 63) == 0) flag[0] = 1;
}

// Stage two, one block over the partials of every group: clip = {total_norm, coef} with
// total_norm = sqrt(sum) * gscale (/ loss scale) and torch.nn.utils.clip_grad_norm_'s
// coef = clamp(max_norm / (total_norm + 1e-6), max = 1), a non-finite norm propagating as there.
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(int npart, const float* __restrict__ part, float gscale,
                                                             const float* __restrict__ amp, float max_norm,
                                                             float* __restrict__ clip, const int* __restrict__ win) {
  if (window_open(win)) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < npart; i += 256) s += (double)part[i];
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double tn = sqrt(red[0]) * (double)gscale;
  if (amp) tn /= (double)amp[0];
  const float total = (float)tn;
  const float c = max_norm / (total + 1e-6f);
  clip[0] = total;
  clip[1] = c > 1.f ? 1.f : c;  // NaN stays NaN (torch.clamp)
}

// AdamW (torch.optim.AdamW semantics, decoupled weight decay) over a flat float32 buffer: the one
// update of every dfm_adamw* entry point. lr and the bias corrections come by value (hyper NULL,
// dfm_adamw) or from device memory, hyper = {lr, step}, so a captured HIP graph replays every step
// without host-baked scalars. With the fp16 loss scaler's device state amp = {scale, growth_tracker,
// applied_steps, skipped} and overflow flag: the step is skipped when flag[0] is set
// (GradScaler.step), gradients are unscaled by 1/scale and the step count is amp[2] + 1 (torch's
// AdamW counts applied steps only).
// OPT = false is that and nothing else: no option is read and g is never written. OPT = true adds
// the options, each a pointer that may be NULL:
//   win    nothing is written unless this is the window's last micro-step
//   clip   the gradient is multiplied by clip[1] (grad_clip_coef_kernel)
//   ema    ema = d * ema + (1 - d) * p_new in the same pass
//   clear_g  g is the accumulation buffer: zero is written back once it is consumed, also by a
//            step that flag skips
// Every rounding is spelled out, so the bits are the source's and not a contraction the compiler
// picks per instantiation (which product of a sum goes into the fma):
//   m = fma(1 - b1, g, rn(b1 m))   v = fma(g, rn((1 - b2) g), rn(b2 v))   p = fma(1 - lr wd, p, -q)
//   q = rn(step_size m) / (sqrt(v) / bc2_sqrt + eps)
template <typename TC, bool OPT>
__global__ void adamw_kernel(long n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ hyper, float lr, float bc1,
                             float bc2_sqrt, float b1, float b2, float eps, float wd, float gscale,
                             TC* __restrict__ copy, const float* __restrict__ amp, const int* __restrict__ flag,
                             const float* __restrict__ clip, const int* __restrict__ win, float* __restrict__ ema,
                             float d, int clear_g) {
  if (OPT && window_open(win)) return;
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  if (flag && flag[0]) {
    if (OPT && clear_g)
      for (long i = t; i < n; i += stride) g[i] = 0.f;
    return;
  }
  if (hyper) {
    const float step = amp ? amp[2] + 1.f : hyper[1];
    lr = hyper[0];
    bc1 = 1.f - powf(b1, step);
    bc2_sqrt = sqrtf(1.f - powf(b2, step));
  }
  if (amp) gscale /= amp[0];
  const float coef = OPT && clip ? clip[1] : 1.f;
  const float decay = __fmaf_rn(-lr, wd, 1.f), step_size = lr / bc1, omb1 = 1.f - b1, omb2 = 1.f - b2, omd = 1.f - d;
  for (long i = t; i < n; i += stride) {
    float gi = __fmul_rn(g[i], gscale);
    if (OPT && clip) gi = __fmul_rn(gi, coef);
    const float mi = __fmaf_rn(omb1, gi, __fmul_rn(b1, m[i]));
    const float vi = __fmaf_rn(gi, __fmul_rn(omb2, gi), __fmul_rn(b2, v[i]));
    m[i] = mi;
    v[i] = vi;
    const float q = __fmul_rn(step_size, mi) / (sqrtf(vi) / bc2_sqrt + eps);
    const float pi = __fmaf_rn(decay, p[i], -q);
    p[i] = pi;
    if (copy) copy[i] = Num<TC>::from_f(pi);
    if (OPT && ema) ema[i] = __fmaf_rn(d, ema[i], __fmul_rn(omd, pi));
    if (OPT && clear_g) g[i] = 0.f;
  }
}

// GradScaler.update (torch/amp/grad_scaler.py _amp_update_scale_) on the loss scaler's device state,
// after the step's AdamW launches have read it; clears the overflow flag for the next step. One
// lane. Inside an accumulation window (win, NULL = no window) the scaler is left alone.
__global__ void loss_scale_update_kernel(float* __restrict__ amp, int* __restrict__ flag, float growth,
                                         float backoff, int interval, const int* __restrict__ win) {
  if (threadIdx.x != 0 || window_open(win)) return;
  if (flag[0]) {
    amp[0] *= backoff;
    amp[1] = 0.f;
    amp[3] += 1.f;
  } else {
    amp[2] += 1.f;
    amp[1] += 1.f;
    if (amp[1] >= (float)interval) {
      amp[0] *= growth;
      amp[1] = 0.f;
    }
  }
  flag[0] = 0;
}

// flag[0] = 1 if any element of g is inf / nan (the GradScaler's found_inf, torch/amp/grad_scaler.py)
__global__ void nonfinite_kernel(long n, const float* __restrict__ g, int* __restrict__ flag) {
  bool bad = false;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    bad |= !isfinite(g[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) flag[0] = 1;
}

// The one AdamW launch, after the entry point's argument checks: OPT = true as soon as one option is on
int adamw_launch(long n, float* p, float* g, float* m, float* v, const float* hyper, float lr, float bc1,
                 float bc2_sqrt, float b1, float b2, float eps, float wd, float gscale, void* copy, int copy_dtype,
                 const float* amp, const int* flag, const float* clip, const int* win, float* ema, float d,
                 int clear_g, dfm_stream_t stream) {
  if (n == 0) return DFM_OK;
  const bool opt = win || clip || ema || clear_g;
  DFM_DTYPE_SWITCH16(copy_code(copy, copy_dtype), TC, {
    const auto kern = opt ? adamw_kernel<TC, true> : adamw_kernel<TC, false>;
    DFM_LAUNCH(kern, dim3(opt_grid(n)), dim3(256), 0, (hipStream_t)stream, n, p, g, m, v, hyper, lr, bc1, bc2_sqrt, b1,
               b2, eps, wd, gscale, (TC*)copy, amp, flag, clip, win, ema, d, clear_g);
  });
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}
}  // namespace

extern "C" int dfm_grad_accumulate(long n, float* acc, const float* g, dfm_stream_t stream) {
  DFM_CHECK_ARG(acc && g && n >= 0, "dfm_grad_accumulate: bad argument");
  if (n == 0) return DFM_OK;
  const long n4 = al16(acc) && al16(g) ? n / 4 : 0;
  DFM_LAUNCH(grad_accumulate_kernel, dim3(opt_grid(n4 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, n, n4, acc, g);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_grad_sumsq_blocks(void) { return SUMSQ_BLOCKS; }

extern "C" int dfm_grad_sumsq(long n, const float* g, float* part, int* flag, const int* win, dfm_stream_t stream) {
  DFM_CHECK_ARG(part && n >= 0 && (g || n == 0), "dfm_grad_sumsq: bad argument");
  const long n4 = al16(g) ? n / 4 : 0;  // n = 0 still launches: the partials must read zero
  DFM_LAUNCH(grad_sumsq_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, (hipStream_t)stream, n, n4, g, part, flag, win);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_grad_clip_coef(int npart, const float* part, float grad_scale, const float* amp, float max_norm,
                                  float* clip_state, const int* win, dfm_stream_t stream) {
  DFM_CHECK_ARG(npart > 0 && part && clip_state && max_norm > 0.f, "dfm_grad_clip_coef: bad argument");
  DFM_LAUNCH(grad_clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, npart, part, grad_scale, amp,
             max_norm, clip_state, win);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_grad_nonfinite(long n, const float* g, int* flag, dfm_stream_t stream) {
  DFM_CHECK_ARG(g && flag && n >= 0, "dfm_grad_nonfinite: bad argument");
  if (n == 0) return DFM_OK;
  DFM_LAUNCH(nonfinite_kernel, dim3(opt_grid(n)), dim3(256), 0, (hipStream_t)stream, n, g, flag);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_adamw(long n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                         float eps, float wd, int step, float gscale, void* copy, int copy_dtype,
                         dfm_stream_t stream) {
  DFM_CHECK_DTYPE16(copy_code(copy, copy_dtype));
  DFM_CHECK_ARG(p && g && m && v && step >= 1, "dfm_adamw: bad argument");
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2 = 1.f - powf(beta2, (float)step);
  return adamw_launch(n, p, const_cast<float*>(g), m, v, nullptr, lr, bc1, sqrtf(bc2), beta1, beta2, eps, wd, gscale,
                      copy, copy_dtype, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, stream);
}

extern "C" int dfm_adamw_dev(long n, float* p, const float* g, float* m, float* v, const float* hyper, float beta1,
                             float beta2, float eps, float wd, float gscale, void* copy, int copy_dtype,
                             dfm_stream_t stream) {
  DFM_CHECK_DTYPE16(copy_code(copy, copy_dtype));
  DFM_CHECK_ARG(p && g && m && v && hyper, "dfm_adamw_dev: bad argument");
  return adamw_launch(n, p, const_cast<float*>(g), m, v, hyper, 0.f, 0.f, 0.f, beta1, beta2, eps, wd, gscale, copy,
                      copy_dtype, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, stream);
}

extern "C" int dfm_adamw_amp(long n, float* p, const float* g, float* m, float* v, const float* hyper,
                             const float* amp, const int* flag, float beta1, float beta2, float eps, float wd,
                             float gscale, void* copy, int copy_dtype, dfm_stream_t stream) {
  DFM_CHECK_DTYPE16(copy_code(copy, copy_dtype));
  DFM_CHECK_ARG(p && g && m && v && hyper && amp && flag, "dfm_adamw_amp: bad argument");
  return adamw_launch(n, p, const_cast<float*>(g), m, v, hyper, 0.f, 0.f, 0.f, beta1, beta2, eps, wd, gscale, copy,
                      copy_dtype, amp, flag, nullptr, nullptr, nullptr, 0.f, 0, stream);
}

extern "C" int dfm_adamw_opt(long n, float* p, float* g, int clear_g, float* m, float* v, const float* hyper,
                             const float* amp, const int* flag, const float* clip_state, const int* win, float* ema,
                             float ema_decay, float beta1, float beta2, float eps, float wd, float gscale,
                             void* copy, int copy_dtype, dfm_stream_t stream) {
  DFM_CHECK_DTYPE16(copy_code(copy, copy_dtype));
  DFM_CHECK_ARG(p && g && m && v && hyper && !amp == !flag, "dfm_adamw_opt: bad argument");
  DFM_CHECK_ARG(!ema || (ema_decay >= 0.f && ema_decay < 1.f), "dfm_adamw_opt: ema_decay %g outside [0, 1)",
                (double)ema_decay);
  return adamw_launch(n, p, g, m, v, hyper, 0.f, 0.f, 0.f, beta1, beta2, eps, wd, gscale, copy, copy_dtype, amp, flag,
                      clip_state, win, ema, ema_decay, clear_g, stream);
}

extern "C" int dfm_loss_scale_update_win(float* amp, int* flag, float growth, float backoff, int interval,
                                         const int* win, dfm_stream_t stream) {
  DFM_CHECK_ARG(amp && flag && interval > 0, "dfm_loss_scale_update_win: bad argument");
  DFM_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, amp, flag, growth, backoff,
             interval, win);
  DFM_LAUNCH_CHECK();
  return DFM_OK;
}

extern "C" int dfm_loss_scale_update(float* amp, int* flag, float growth, float backoff, int interval,
                                     dfm_stream_t stream) {
  DFM_CHECK_ARG(amp && flag && interval > 0, "dfm_loss_scale_update: bad argument");
  return dfm_loss_scale_update_win(amp, flag, growth, backoff, interval, nullptr, stream);
}
