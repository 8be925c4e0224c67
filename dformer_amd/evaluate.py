"""Multi-scale + flip evaluation and mIoU metrics on the HIP path.

The reference's `utils/val_mm.py` (`evaluate_msf` 325-472, `slide_inference` 257-322, `evaluate`
102-207, `save_preds` 25-98) and `utils/metrics_new.py:6-47 Metrics`, same names, arguments and
results. Everything after the model works on the decoder's low-res logits as NHWC rows:
- `evaluate_msf`: per scale [and flip] one kernel folds the model's upsampling (align_corners=False),
  the flip back, the resize to the label size (align_corners=True), the softmax and the sum over
  scales into a float32 [B*H*W, ncls] buffer. With `sliding=True` the scaled image is cut into crops
  of `config.eval_crop_size` at a stride of int(`config.eval_stride_rate` * crop), the crops run
  through the model in stacks, and the same kernel averages the covering windows per label pixel.
  `save_dir` raises.
- `evaluate` / `save_preds`: `K.seg_predict` turns the low-res logits into the uint8 class map and
  the confusion histogram; with `sliding=True` the window-averaged logits go through `update_rows` /
  `K.rows_argmax`.
No full-resolution logits, zero-padded windows, sum or count maps are materialised.
"""
import collections
import math
import os

import torch

from . import kernels as K


class Metrics:
    """utils/metrics_new.py:6-47: confusion histogram over labelled pixels, IoU / F1 / accuracy."""

    def __init__(self, num_classes, ignore_label, device):
        self.ignore_label = ignore_label
        self.num_classes = num_classes
        self._hist = torch.zeros(num_classes * num_classes, dtype=torch.int64, device=device)
        self.index = 0

    @property
    def hist(self):
        return self._hist.view(self.num_classes, self.num_classes).float()

    def update_hist(self, hist):
        self._hist += hist.to(self._hist.device).reshape(-1).round().long()

    def update_rows(self, acc, target):
        """acc: float32 [B*H*W, ncls] class scores (NHWC rows), target: [B, H, W] labels."""
        self.index += 1
        K.seg_confusion(acc, target.long().contiguous(), self.num_classes, self.ignore_label, self._hist)

    def update(self, pred, target):
        """pred: [B, ncls, H, W] class scores (any layout), target: [B, H, W]."""
        rows = pred.float().permute(0, 2, 3, 1).contiguous().view(-1, pred.shape[1])
        self.update_rows(rows, target)

    def update_low(self, low_rows, shape, target, pred=None):
        """The fused update from the decoder's low-res logits: low_rows [B*h*w, >= ncls] NHWC rows,
        shape = (B, h, w), target [B, H, W]. Equals update(F.interpolate(low, (H, W), 'bilinear',
        align_corners=False), target) without materialising the upsampled logits; pred (uint8
        [B, H, W], optional) receives the class map."""
        B, h, w = shape
        if target.dim() != 3 or target.shape[0] != B:
            raise ValueError(f"update_low: target {tuple(target.shape)} is not [{B}, H, W]")
        self.index += 1
        K.seg_predict(low_rows, B, h, w, self.num_classes, tuple(target.shape[1:]), pred=pred,
                      label=target.long().contiguous(), ignore=self.ignore_label, hist=self._hist)
        return pred

    def compute_iou(self):
        h = self.hist
        ious = h.diag() / (h.sum(0) + h.sum(1) - h.diag())
        ious[ious.isnan()] = 0.0
        miou = ious.mean().item()
        ious *= 100
        miou *= 100
        return ious.cpu().numpy().round(2).tolist(), round(miou, 2)

    def compute_f1(self):
        h = self.hist
        f1 = 2 * h.diag() / (h.sum(0) + h.sum(1))
        f1[f1.isnan()] = 0.0
        mf1 = f1.mean().item()
        f1 *= 100
        mf1 *= 100
        return f1.cpu().numpy().round(2).tolist(), round(mf1, 2)

    def compute_pixel_acc(self):
        h = self.hist
        acc = h.diag() / h.sum(1)
        acc[acc.isnan()] = 0.0
        macc = acc.mean().item()
        acc *= 100
        macc *= 100
        return acc.cpu().numpy().round(2).tolist(), round(macc, 2)


def msf_size(H, W, scale):
    """val_mm.py:359-364: the scaled input size, rounded up to a multiple of 32."""
    nh, nw = int(scale * H), int(scale * W)
    return int(math.ceil(nh / 32)) * 32, int(math.ceil(nw / 32)) * 32


def slide_windows(n, crop, stride):
    """val_mm.py:295-306: the (start, end) of every sliding window along an axis of n pixels; the last
    window is moved back so that it ends at n."""
    out = []
    for i in range(K.slide_grids(n, crop, stride)):
        end = min(i * stride + crop, n)
        out.append((max(end - crop, 0), end))
    return out


def slide_strides(crop_size, stride_rate):
    """val_mm.py:288-291: (h_stride, w_stride) = int(rate * crop) per axis."""
    strides = tuple(int(stride_rate * c) for c in crop_size)
    if min(strides) <= 0:
        raise ValueError(f"sliding-window stride int({stride_rate} * {tuple(crop_size)}) = {strides} must be positive")
    if strides[0] > crop_size[0] or strides[1] > crop_size[1]:
        raise ValueError(f"sliding-window stride {strides} exceeds the crop {tuple(crop_size)}: pixels between "
                         f"windows would get no prediction")
    return strides


def _optional(config, name):
    try:  # a dict-backed config raises KeyError for a missing name
        return getattr(config, name)
    except (AttributeError, KeyError):
        return None


# the crop (hc, wc), its strides (slide_strides) and the most images per model call (None: one window of the batch)
_Slide = collections.namedtuple("_Slide", "crop strides crop_batch")


def _slide_config(config, crop_size=None, stride_rate=None, crop_batch=None):
    """The validated sliding-window settings: config's eval_crop_size, eval_stride_rate and (optional)
    eval_crop_batch, or, without a config, the arguments."""
    if config is not None:
        crop_size, stride_rate = config.eval_crop_size, config.eval_stride_rate
        crop_batch = _optional(config, "eval_crop_batch")
    crop = tuple(int(c) for c in crop_size)
    return _Slide(crop, slide_strides(crop, stride_rate), crop_batch)


def _scan_model(model):
    """True when the model's modal_x is a laser scan (the DFormerTrav backbone), not a depth image."""
    return bool(getattr(getattr(model, "encoder_backbone", None), "scan_input", False))


def _no_scan(model, what):
    """A scan [B, 1, N] cannot be resized, cropped or flipped with the image. The reference does nothing
    definite there: slide_inference asserts equal image / modal_x sizes (val_mm.py:293) and evaluate_msf
    interpolates and flips modal_x as a 4-D image (val_mm.py:362-372, 386-388), both of which fail on a scan."""
    if _scan_model(model):
        raise NotImplementedError(f"{what}: the DFormerTrav backbone reads a laser scan, which cannot be resized, "
                                  "cropped or flipped; evaluate at scale 1 without flip or sliding windows")


def _slide_low_rows(model, x, e, slide):
    """The low-res logits of every sliding window of the scaled (and flipped) inputs x, e:
    ([G*B*h*w, ncls] rows, window-major, (B, h, w), (Hs, Ws) of the image the windows were cut from)."""
    _no_scan(model, "sliding-window inference")
    hc, wc = slide.crop
    if hc > x.shape[2] or wc > x.shape[3]:  # val_mm.py:280-286: both dimensions go to the crop size
        x = K.resize_nchw(x, (hc, wc), True)
        e = K.resize_nchw(e, (hc, wc), True)
    B, _, Hs, Ws = x.shape
    wins = [(y1, y2, x1, x2) for y1, y2 in slide_windows(Hs, hc, slide.strides[0])
            for x1, x2 in slide_windows(Ws, wc, slide.strides[1])]
    per = max(1, (slide.crop_batch if slide.crop_batch is not None else B) // B)  # whole windows per model call
    buf, shape, off = None, None, 0
    for i in range(0, len(wins), per):
        chunk = wins[i:i + per]
        cx = torch.cat([x[:, :, y1:y2, x1:x2] for y1, y2, x1, x2 in chunk], 0)
        ce = torch.cat([e[:, :, y1:y2, x1:x2] for y1, y2, x1, x2 in chunk], 0)
        rows, (b, h, w) = model._low_rows(cx, ce)
        if buf is None:
            shape = (B, h, w)
            buf = torch.empty(len(wins) * B * h * w, rows.shape[1], device=rows.device, dtype=rows.dtype)
        buf[off:off + b * h * w].copy_(rows)
        off += b * h * w
    return buf, shape, (Hs, Ws)


@torch.no_grad()
def msf_scores(model, rgb, modal_x, num_classes, scales, flip, out_shape=None, crop_size=None, stride_rate=None,
               crop_batch=None, slide=None):
    """Summed softmax scores over scales (and flips) of one batch: float32 [B*H*W, ncls] rows
    (val_mm.py:355-392 for one batch; `scaled_logits` of the reference, channels last). Like the
    reference (val_mm.py:355-356) the scaled sizes and the score buffer follow the LABEL's
    (B, H, W) = out_shape (default: the image's own size).

    With crop_size = (hc, wc) every scale runs the reference's sliding-window inference: windows of
    crop_size at a stride of int(stride_rate * crop), at most crop_batch images (default: one window
    of the batch) per model call. slide is the same as a validated record (evaluate_msf's)."""
    B, H, W = out_shape if out_shape is not None else (rgb.shape[0], rgb.shape[2], rgb.shape[3])
    if rgb.shape[0] != B or modal_x.shape[0] != B:
        raise ValueError(f"msf_scores: batch of the images {rgb.shape[0]} != labels {B}")
    if crop_size is not None:
        slide = _slide_config(None, crop_size, stride_rate, crop_batch)
    scan = _scan_model(model)
    if scan and (slide is not None or flip or any(msf_size(H, W, s) != (H, W) for s in scales)):
        _no_scan(model, "multi-scale / flip / sliding-window evaluation")
    acc = torch.zeros(B * H * W, num_classes, device=rgb.device, dtype=torch.float32)
    for scale in scales:
        size = msf_size(H, W, scale)
        for f in ((False, True) if flip else (False,)):
            x = K.resize_nchw(rgb, size, True, flip=f)
            e = modal_x if scan else K.resize_nchw(modal_x, size, True, flip=f)
            if slide is not None:
                rows, (b, h, w), scaled = _slide_low_rows(model, x, e, slide)
                K.slide_msf_accumulate(rows, b, h, w, num_classes, slide.crop, slide.strides, scaled, (H, W), f, acc)
                continue
            rows, (b, h, w) = model._low_rows(x, e)
            K.msf_accumulate(rows, b, h, w, num_classes, size, (H, W), f, acc)
    return acc


def _slide_rows(model, imgs, modal_xs, ncls, slide):
    """slide_inference as NHWC rows: (float32 [B*Hs'*Ws', ncls], (B, Hs', Ws'))."""
    rows, (b, h, w), (Hs, Ws) = _slide_low_rows(model, imgs, modal_xs, slide)
    out = torch.empty(b * Hs * Ws, ncls, device=rows.device, dtype=torch.float32)
    K.slide_msf_accumulate(rows, b, h, w, ncls, slide.crop, slide.strides, (Hs, Ws), (Hs, Ws), False, out,
                           softmax=False)
    return out, (b, Hs, Ws)


@torch.no_grad()
def slide_inference(model, imgs, modal_xs, config, crop_batch=None):
    """val_mm.py:257-322: the window-averaged logits of imgs, float32 [B, ncls, Hs', Ws'] (an NCHW
    view of NHWC rows), (Hs', Ws') the image size after the reference's up-sizing to the crop."""
    slide = _slide_config(config)._replace(crop_batch=crop_batch)
    out, shape = _slide_rows(model, imgs, modal_xs, config.num_classes, slide)
    return out.view(*shape, -1).permute(0, 3, 1, 2)


def pred_png_name(fn):
    """val_mm.py:161-167: the path of a prediction image below save_dir, without the "_pred.png"."""
    return fn.replace(".jpg", "").replace(".png", "").replace("datasets/", "")


def pred_img_id(rgb_path):
    """val_mm.py:89: the last path component with leading and trailing '.', 'j', 'p', 'g' characters
    removed (str.strip('.jpg') strips a character set, not a suffix; the reference's file names are
    the contract)."""
    return rgb_path.split("/")[-1].strip(".jpg")


def check_palette(palette, num_classes):
    """The caller's colour table as a uint8 [>= num_classes, 3] numpy array."""
    import numpy as np
    pal = palette.detach().cpu().numpy() if isinstance(palette, torch.Tensor) else np.asarray(palette)
    if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < num_classes:
        raise ValueError(f"palette of shape {pal.shape} is not [>= {num_classes}, 3]")
    if pal.dtype != np.uint8:
        if not np.issubdtype(pal.dtype, np.integer) or pal.min() < 0 or pal.max() > 255:
            raise ValueError(f"palette values must be integers in [0, 255], got {pal.dtype}")
        pal = pal.astype(np.uint8)
    return pal


def _write_pred_png(path, pred, palette):
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("evaluate(save_dir=...) writes PNG files with Pillow (PIL), which is not installed") from e
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(pred if palette is None else palette[pred]).save(path)


def _batch_inputs(batch, device, scan=False):
    """val_mm.py:41-52, 115-125: rgb, depth ('laser', the reference's key here, else 'modal_x') and gt of
    a batch on the device; an unbatched sample gets its batch axis. scan: modal_x holds laser scans
    (DFormerTrav), one per image: [B, 1, N] whatever axes the loader gave it."""
    rgb, gt = batch["rgb"], batch["gt"]
    modal_x = batch["laser"] if "laser" in batch else batch["modal_x"]
    if rgb.dim() == 3:
        rgb = rgb.unsqueeze(0)
    if scan:
        modal_x = modal_x.reshape(rgb.shape[0], 1, -1)
    elif modal_x.dim() == 3:
        modal_x = modal_x.unsqueeze(0)
    if gt.dim() == 2:
        gt = gt.unsqueeze(0)
    return rgb.to(device), modal_x.to(device), gt.to(device)


def _run(model, dataloader, config, device, engine, sliding, step):
    """The loop of evaluate_msf, evaluate and save_preds: step(metrics, slide, batch, rgb, modal_x, gt) per
    batch, slide being config's sliding-window settings (None unless sliding). Returns the Metrics (a list
    of every rank's Metrics when engine.distributed, like the reference)."""
    if sliding:
        _no_scan(model, "sliding-window evaluation")
    slide = _slide_config(config) if sliding else None  # a bad rate fails before the first batch
    model.eval()
    metrics = Metrics(config.num_classes, config.background, device)
    scan = _scan_model(model)
    for batch in dataloader:
        step(metrics, slide, batch, *_batch_inputs(batch, device, scan))
    if engine is not None and getattr(engine, "distributed", False):
        all_metrics = [None for _ in range(engine.world_size)]
        torch.distributed.all_gather_object(all_metrics, metrics)
        return all_metrics
    return metrics


@torch.no_grad()
def evaluate_msf(model, dataloader, config, device, scales, flip, engine=None, save_dir=None, sliding=False):
    """val_mm.py:325-472. dataloader yields dicts with 'rgb', 'modal_x' (or 'laser'), 'gt'. Returns the
    Metrics (a list of every rank's Metrics when engine.distributed, like the reference). sliding=True
    runs every scale through sliding-window inference with config.eval_crop_size and
    config.eval_stride_rate (and config.eval_crop_batch images per model call, when set)."""
    if save_dir is not None:
        raise NotImplementedError("evaluate_msf: prediction image export is outside the hot path (SURVEY.md §2)")

    def step(metrics, slide, batch, rgb, modal_x, gt):
        acc = msf_scores(model, rgb, modal_x, config.num_classes, scales, flip, out_shape=tuple(gt.shape), slide=slide)
        metrics.update_rows(acc, gt)

    return _run(model, dataloader, config, device, engine, sliding, step)


def _update_batch(model, metrics, slide, rgb, modal_x, gt, want_pred):
    """One batch of evaluate / save_preds: the histogram update and, when asked for, the uint8 class map
    [B, H, W] (on the device)."""
    if slide is not None:
        rows, shape = _slide_rows(model, rgb, modal_x, metrics.num_classes, slide)
        if shape[1:] != tuple(gt.shape[-2:]):
            raise ValueError(f"evaluate: sliding-window predictions {shape[1:]} do not match the labels "
                             f"{tuple(gt.shape[-2:])}")
        metrics.update_rows(rows, gt)
        return K.rows_argmax(rows, metrics.num_classes).view(gt.shape) if want_pred else None
    if tuple(gt.shape[-2:]) != tuple(rgb.shape[-2:]):
        raise ValueError(f"evaluate: labels {tuple(gt.shape[-2:])} do not match the image {tuple(rgb.shape[-2:])}")
    rows, shape = model._low_rows(rgb, modal_x)
    pred = torch.empty(gt.shape, device=rows.device, dtype=torch.uint8) if want_pred else None
    return metrics.update_low(rows, shape, gt, pred=pred)


@torch.no_grad()
def evaluate(model, dataloader, config, device, engine=None, save_dir=None, sliding=False, palette=None):
    """val_mm.py:102-207. dataloader yields dicts with 'rgb', 'laser' (or 'modal_x'), 'gt' and, for
    save_dir, 'fn'. Returns the Metrics (a list of every rank's Metrics when engine.distributed).
    save_dir writes <save_dir>/<name>_pred.png for every image of a batch: coloured with `palette`
    (else config.palette; uint8 [>= num_classes, 3], the caller's data) or, without one, the class
    indices as an 8-bit image."""
    if save_dir is not None:
        if palette is None:
            palette = _optional(config, "palette")
        if palette is not None:
            palette = check_palette(palette, config.num_classes)

    def step(metrics, slide, batch, rgb, modal_x, gt):
        pred = _update_batch(model, metrics, slide, rgb, modal_x, gt, save_dir is not None)
        if save_dir is not None:
            for p, fn in zip(pred.cpu().numpy(), batch["fn"]):
                _write_pred_png(os.path.join(save_dir, pred_png_name(fn) + "_pred.png"), p, palette)

    return _run(model, dataloader, config, device, engine, sliding, step)


FSS_KEYS = ("s_img", "s_depth", "s_gt", "q_img", "q_depth", "q_gt")


def _episode_inputs(batch, device):
    """val_mm.py:222-227: the six tensors of an episode batch on the device, in meta_forward's order plus q_gt."""
    missing = [k for k in FSS_KEYS if k not in batch]
    if missing:
        raise KeyError(f"fss_evaluate: the batch lacks {missing} (it has {sorted(batch)})")
    return tuple(batch[k].to(device) for k in FSS_KEYS)


@torch.no_grad()
def fss_evaluate(model, dataloader, config, device, engine=None, save_dir=None, palette=None):
    """val_mm.py:210-254: eval-mode meta_forward per episode batch (keys s_img, s_gt, s_depth, q_img, q_gt,
    q_depth and, for save_dir, fn), the fused score rows counted against q_gt. Returns the Metrics (a list of
    every rank's when engine.distributed). save_dir writes <save_dir>/<name>_pred.png per query image:
    coloured with `palette` (else config.palette), or the class indices as an 8-bit image."""
    if save_dir is not None:
        if palette is None:
            palette = _optional(config, "palette")
        if palette is not None:
            palette = check_palette(palette, config.num_classes)
    model.eval()
    metrics = Metrics(config.num_classes, config.background, device)
    for batch in dataloader:
        s_rgb, s_depth, s_gt, q_rgb, q_depth, q_gt = _episode_inputs(batch, device)
        logits = model.meta_forward(s_rgb, s_depth, s_gt, q_rgb, q_depth)  # an NCHW view of [B*H*W, 2] rows
        if tuple(q_gt.shape) != (logits.shape[0],) + tuple(logits.shape[-2:]):
            raise ValueError(f"fss_evaluate: q_gt {tuple(q_gt.shape)} does not match the logits {tuple(logits.shape)}")
        rows = logits.permute(0, 2, 3, 1).reshape(-1, logits.shape[1])
        metrics.update_rows(rows, q_gt)
        if save_dir is not None:
            pred = K.rows_argmax(rows, config.num_classes).view(q_gt.shape)
            for p, fn in zip(pred.cpu().numpy(), batch["fn"]):
                _write_pred_png(os.path.join(save_dir, pred_png_name(fn) + "_pred.png"), p, palette)
    if engine is not None and getattr(engine, "distributed", False):
        all_metrics = [None for _ in range(engine.world_size)]
        torch.distributed.all_gather_object(all_metrics, metrics)
        return all_metrics
    return metrics


@torch.no_grad()
def save_preds(model, dataloader, config, device, engine=None, model_path=None, sliding=False, out_root="output"):
    """val_mm.py:25-98: the metrics of `evaluate` plus one <out_root>/<model_path>/<img_id>.npy uint8 class
    map per image, img_id from batch['rgb_path'][i] (pred_img_id)."""
    import numpy as np
    out_dir = os.path.join(out_root, str(model_path))

    def step(metrics, slide, batch, rgb, modal_x, gt):
        pred = _update_batch(model, metrics, slide, rgb, modal_x, gt, True)
        os.makedirs(out_dir, exist_ok=True)
        for p, path in zip(pred.cpu().numpy(), batch["rgb_path"]):
            np.save(os.path.join(out_dir, pred_img_id(path) + ".npy"), p)

    return _run(model, dataloader, config, device, engine, sliding, step)
