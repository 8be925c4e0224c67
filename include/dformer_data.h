/* dformer_data.h — C ABI of libdformer_data.so: the training-input preprocessing of DFormer's loader
 * (utils/dataloader/dataloader.py:20-76 TrainPre, 112-122 ValPre in Originofamonia/DFormer) as one
 * gfx950 kernel over a batch of raw uint8 images.
 *
 * The library is separate from libdformer_hip.so (include/dformer_hip.h): the model never calls it and a
 * host that feeds ready tensors never loads it. The contract is the model library's:
 *   - plain device pointers + sizes; no torch types;
 *   - the caller owns every buffer; the call never allocates, never synchronises the host and only
 *     enqueues on `stream` (a hipStream_t passed as void*; NULL = default stream), so it can be captured
 *     into a HIP graph;
 *   - return 0 on success, negative on bad arguments / launch failure; dfd_last_error() returns a
 *     thread-local message for the last failure. Arguments are validated before anything is launched.
 */
#ifndef DFORMER_DATA_H
#define DFORMER_DATA_H

#ifdef __cplusplus
extern "C" {
#endif

#define DFD_OK 0
#define DFD_ERR_ARG (-1)
#define DFD_ERR_LAUNCH (-3)

/* Limits: raw and crop sizes up to DFD_MAX_DIM per side, scaled sizes (sh, sw) up to DFD_MAX_SCALED.
 * They keep every index product of the kernel inside 31 bits. */
#define DFD_MAX_DIM 16384
#define DFD_MAX_SCALED 32768

typedef void* dfd_stream_t;

const char* dfd_last_error(void);
int dfd_abi_version(void); /* 1: dfd_train_pre */

/* One batch: every sample has the raw size H0 x W0 (one size per call) and is written as a ch x cw crop.
 * modal_channels is 1 ([B,H0,W0] uint8) or 3 ([B,H0,W0,3] uint8). bgr != 0: the rgb source (and a
 * 3-channel modal source) is stored B,G,R; output plane c then reads source channel 2 - c.
 * transform_gt != 0: the label is stored as (g - 1) & 255 (RGBXDataset._gt_transform on uint8).
 * mean / std normalise the rgb planes, modal_mean / modal_std the modal planes (a 1-channel modal
 * uses element 0); every std must be > 0. */
typedef struct {
  int B, H0, W0;
  int ch, cw;
  int modal_channels;
  int bgr, transform_gt;
  float mean[3], std[3];
  float modal_mean[3], modal_std[3];
} DfdPreDesc;

/* TrainPre for a batch in one launch: mirror, resize, normalise, crop and pad.
 *   rgb   [B,H0,W0,3] uint8      modal [B,H0,W0] or [B,H0,W0,3] uint8      gt [B,H0,W0] uint8
 *   params [B,8] int32, rows (flip, sh, sw, pos_h, pos_w, 0, 0, 0): mirror flag (non-zero = mirror), the
 *          scaled size and the crop's top-left corner in the scaled image
 *   out_rgb [B,3,ch,cw] float32   out_modal [B,modal_channels,ch,cw] float32   out_label [B,ch,cw] int64
 * Output pixel (y, x) of sample b: hc = clamp(sh - pos_h, 0, ch), wc = clamp(sw - pos_w, 0, cw),
 * pt = (ch - hc) / 2, pl = (cw - wc) / 2 (pad_image_to_shape, transforms.py:61-75: the smaller half on top
 * and on the left), yy = y - pt, xx = x - pl. Outside 0 <= yy < hc, 0 <= xx < wc the images are 0.0
 * (after normalisation, as the reference pads) and the label is 255. Inside, (r, c) = (pos_h + yy,
 * pos_w + xx) is the pixel of the scaled image.
 *   images: bilinear with half-pixel centres (cv2.INTER_LINEAR's mapping) from exact integers: rows
 *     num = (2r+1) H0 - sh, den = 2 sh, s0 = floor(num / den), w = (num - s0 den) / den; num < 0 gives
 *     (s0, w) = (0, 0), s0 >= H0-1 gives (H0-1, 0); second tap min(s0+1, H0-1); columns alike with W0, sw,
 *     and a mirrored sample reads source column W0-1-s for column tap s. The uint8 taps are combined in
 *     float32, q = floor(v + 0.5) (the reference's resize returns uint8) and out = (q/255 - mean)/std.
 *     sh == H0 and sw == W0 is exact (every weight 0).
 *   label: nearest (cv2.INTER_NEAREST's mapping): source row min(r H0 / sh, H0-1), source column
 *     min(c W0 / sw, W0-1), mirrored as above.
 * Memory safety does not depend on `params` (they may be device data nobody has read): every source
 * index is clamped to the raw image, r < 0 or c < 0 reads row / column tap 0, and a row with sh <= 0,
 * sw <= 0, sh > DFD_MAX_SCALED or sw > DFD_MAX_SCALED yields padding only.
 * Rejected with DFD_ERR_ARG before any launch: a null pointer, B / H0 / W0 / ch / cw <= 0, H0 / W0 / ch /
 * cw > DFD_MAX_DIM, modal_channels not 1 or 3, a std that is not > 0. */
int dfd_train_pre(const DfdPreDesc* desc, const void* rgb, const void* modal, const void* gt, const void* params,
                  void* out_rgb, void* out_modal, void* out_label, dfd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
