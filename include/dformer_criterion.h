/* dformer_criterion.h — C ABI of libdformer_criterion.so: the focal and Tversky / Dice terms of the
 * segmentation criterion (losses.FusedSegLoss with focal_gamma / region) on the low-resolution logits of a
 * decode head, fused with the bilinear upsample to the label size: the full-resolution logits are never
 * materialised.
 *
 * The library is separate from libdformer_hip.so (include/dformer_hip.h): a training run with the default
 * criterion never loads it. The contract is the model library's:
 *   - plain device pointers + sizes; no torch types;
 *   - the caller owns every buffer; a call never allocates, never synchronises the host, never reads device
 *     memory on the host and only enqueues on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream), so it can be captured into a HIP graph;
 *   - return 0 on success, negative on bad arguments / launch failure; dfc_last_error() returns a
 *     thread-local message for the last failure. Arguments are validated before anything is launched.
 *
 * Definitions. Let z = up(logits) be the bilinear upsample (half-pixel centres, align_corners=False, the tap
 * rule of dfm_seg_loss_fwd) of logits [B, h, w, ncls] to the label size H x W, p = softmax(z) over the
 * classes, v_i = [label_i != ignore and 0 <= label_i < ncls], w the class weights (all 1 if NULL).
 *   pixel term   sum_i v_i w[y_i] (1 - p_{i,y_i})^gamma (-log p_{i,y_i})            (gamma = 0: cross-entropy)
 *   per image b and class c:  TP = sum_i v_i p_ic [y_i = c],  SP = sum_i v_i p_ic,  SY = sum_i v_i [y_i = c]
 *   T_bc = (TP + s) / (TP + alpha (SP - TP) + beta (SY - TP) + s)
 *   L_reg = 1 / (B ncls) sum_b sum_c w[c] (1 - T_bc)
 * All arithmetic is float32; every sum has a fixed order (no floating-point atomics): a second call on the
 * same inputs gives the same bits.
 */
#ifndef DFORMER_CRITERION_H
#define DFORMER_CRITERION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFC_OK 0
#define DFC_ERR_ARG (-1)
#define DFC_ERR_LAUNCH (-3)

#define DFC_F32 0
#define DFC_BF16 1
#define DFC_F16 2

#define DFC_MAX_CLASSES 64
#define DFC_MAX_DIM 16384 /* h, w, H, W per side */
#define DFC_MAX_BATCH 65535

typedef void* dfc_stream_t;

const char* dfc_last_error(void);
int dfc_abi_version(void); /* 1: dfc_seg_terms_workspace, dfc_seg_terms_fwd, dfc_seg_terms_bwd */

/* Which terms a call computes. has_pixel = 0 leaves the pixel term out (its sum is written as 0 and it
 * adds nothing to the gradient; the valid count is still written); has_region = 0 leaves the region term
 * out (stats and L_reg are written as 0). gamma >= 0; alpha, beta >= 0 with alpha + beta > 0 and smooth > 0
 * are required only with has_region. */
typedef struct {
  float gamma;
  float alpha, beta, smooth;
  int has_pixel, has_region;
} DfcTermsDesc;

/* bytes of `workspace` for dfc_seg_terms_fwd (block partials; the backward needs none); 0 on bad sizes */
size_t dfc_seg_terms_workspace(int B, int h, int w, int ncls, int H, int W);

/* logits [B*h*w, ncls] in dtype, label int64 [B, H, W], weight float32 [ncls] or NULL.
 *   stats float32 [B, ncls, 3] = (TP, SP, SY) per image and class
 *   out   float32 [3]          = (pixel-term sum, valid-pixel count, L_reg)
 * Rejected with DFC_ERR_ARG before any launch: an unknown dtype, B / h / w / H / W / ncls <= 0 or above
 * their limits, h > H or w > W, a null desc / logits / label / workspace / stats / out, gamma < 0 or not
 * finite, and with has_region: smooth <= 0, alpha < 0, beta < 0, alpha + beta <= 0. */
int dfc_seg_terms_fwd(int dtype, int B, int h, int w, int ncls, const void* logits, int H, int W,
                      const void* label, int ignore, const float* weight, const DfcTermsDesc* desc,
                      void* workspace, float* stats, float* out, dfc_stream_t stream);

/* dlogits [B*h*w, ncls] in dtype = gscale * d(out[0] / max(out[1], 1) + region_weight * out[2]) / d logits:
 * every element is written, each as a fixed-order sum over the label pixels whose bilinear taps touch its
 * cell. stats and out are the forward's; gscale is a device float32 [1] (the upstream gradient, which
 * carries a loss scale), NULL = 1. Rejected as in dfc_seg_terms_fwd, and: null stats / out / dlogits,
 * region_weight < 0 or not finite. */
int dfc_seg_terms_bwd(int dtype, int B, int h, int w, int ncls, const void* logits, int H, int W,
                      const void* label, int ignore, const float* weight, const DfcTermsDesc* desc,
                      const float* stats, const float* out, const float* gscale, float region_weight,
                      void* dlogits, dfc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
