"""Criteria of the fused segmentation loss.

FusedSegLoss is the criterion EncoderDecoder takes when the plain CrossEntropyLoss of utils/train.py:189-194
is not enough: class weights and label smoothing (the nn.CrossEntropyLoss arguments, builder.py:230) and
online hard example mining (utils/loss_opr.py:137-187, ProbOhemCrossEntropy2d). Inside the segmentor the
options go to the fused HIP loss (decoders.SegLossFn): the full-resolution logits are never materialised.
Called directly on full-resolution logits, forward() below is the same definition in plain torch ops.

Not taken over from ProbOhemCrossEntropy2d: its `use_weight` table of 19 Cityscapes class weights (pass
`weight=`) and `down_ratio` (its own forward never reads it).

focal_gamma and region add the two families the reference ships for imbalanced segmentation: a focal loss
(utils/loss_opr.py:12-23 FocalLoss2d, models/losses/focal_loss.py) and the Tversky / Dice region losses
(models/losses/tversky_loss.py, dice_loss.py). Inside the segmentor they run on the fused kernels of
dformer_amd.criterion (libdformer_criterion.so), which is imported on their first use: a default criterion
loads and launches nothing new.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

MAX_CLASSES = 64  # the loss kernels hold one pixel's class row in registers


class FusedSegLoss(nn.Module):
    """loss = sum_{i in K} l_i / max(|K|, 1) with, per pixel i of label y_i and C classes,

        l_i = (1 - eps) w[y_i] (-log p_{i,y_i}) + eps / C sum_c w[c] (-log p_{i,c})

    which is F.cross_entropy(pred, target, weight=w, reduction='none', ignore_index=ignore_index,
    label_smoothing=eps)[i], and K the kept pixels. The denominator is the pixel COUNT |K|, not the sum of the
    weights: that is what the reference's `criterion(out, label)[label != background].mean()` (builder.py:230)
    gives for a criterion with reduction='none', and it differs from nn.CrossEntropyLoss(weight=w,
    reduction='mean'), which divides by sum_i w[y_i].

    Kept set: without mining (ohem_thresh None) the valid pixels (target != ignore_index). With mining
    (loss_opr.py:157-185), p_i being the softmax probability of the true class: if ohem_min_kept == 0 or
    ohem_min_kept > num_valid nothing is mined (loss_opr.py:174, 167); otherwise threshold = max(ohem_thresh,
    the ohem_min_kept-th smallest p_i over the valid pixels) and K = {valid i : p_i <= threshold}, ties kept.
    The selection carries no gradient.

    weight: one non-negative entry per output channel of the head the criterion is applied to (None = 1).

    Focal term. With focal_gamma = g > 0 the pixel term above is replaced by, v_i = [y_i != ignore_index],

        L_pix = sum_i v_i w[y_i] (1 - p_{i,y_i})^g (-log p_{i,y_i}) / max(sum_i v_i, 1)

    the usual focal loss, normalised by the valid-pixel count like every loss here. The reference's FocalLoss2d
    (loss_opr.py:12-23) hard-codes the exponent 2 whatever its `gamma`; that quirk is not taken over. Label
    smoothing and mining are not defined together with focal_gamma > 0 and are rejected.

    Region term. With region = "tversky" (region_alpha a, region_beta b, None = 0.3 / 0.7; region_smooth s) or
    "dice" (a = b = 0.5, the soft Dice coefficient; it takes no region_alpha / region_beta), per image b and class c over the valid pixels of the ORIGINAL labels (mining
    selects pixels for the pixel term only):

        TP = sum_i v_i p_ic [y_i = c],  FP = sum_i v_i p_ic - TP,  FN = sum_i v_i [y_i = c] - TP
        T_bc = (TP + s) / (TP + a FP + b FN + s)
        L_reg = mean_b 1/C sum_c w[c] (1 - T_bc)

    as models/losses/tversky_loss.py:14-57 (valid mask, per image, summed over classes, divided by C, mean over
    the batch). mmseg's DiceLoss (dice_loss.py:44-45, 108-110) squares the denominator's terms and does not mask
    it, so ignored pixels count towards class C - 1 through its clamp; that is not reproduced.

    loss = pixel term + region_weight * L_reg.
    """

    def __init__(self, ignore_index=255, weight=None, label_smoothing=0.0, ohem_thresh=None, ohem_min_kept=0,
                 focal_gamma=0.0, region=None, region_weight=1.0, region_alpha=None, region_beta=None,
                 region_smooth=1.0):
        super().__init__()
        self.ignore_index = int(ignore_index)
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"FusedSegLoss: label_smoothing {label_smoothing} is not in [0, 1)")
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().clone().contiguous()
            if weight.dim() != 1 or not 1 <= weight.numel() <= MAX_CLASSES:
                raise ValueError(f"FusedSegLoss: weight {tuple(weight.shape)} is not a vector of 1..{MAX_CLASSES} "
                                 "class weights")
            if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
                raise ValueError("FusedSegLoss: class weights must be finite and non-negative")
        # not persistent: the segmentor's state_dict keeps the reference's keys
        self.register_buffer("weight", weight, persistent=False)
        self.ohem_thresh = None if ohem_thresh is None else float(ohem_thresh)
        if self.ohem_thresh is not None and not 0.0 <= self.ohem_thresh <= 1.0:
            raise ValueError(f"FusedSegLoss: ohem_thresh {ohem_thresh} is not a probability")
        self.ohem_min_kept = int(ohem_min_kept)
        if self.ohem_min_kept < 0:
            raise ValueError(f"FusedSegLoss: ohem_min_kept {ohem_min_kept} is negative")
        self.focal_gamma = float(focal_gamma)
        if not (math.isfinite(self.focal_gamma) and self.focal_gamma >= 0.0):
            raise ValueError(f"FusedSegLoss: focal_gamma {focal_gamma} is not a finite number >= 0")
        if self.focal_gamma > 0.0 and (self.label_smoothing != 0.0 or self.ohem_thresh is not None):
            raise ValueError("FusedSegLoss: focal_gamma > 0 is not defined together with label_smoothing or "
                             "ohem_thresh")
        if region not in (None, "tversky", "dice"):
            raise ValueError(f"FusedSegLoss: region {region!r} is not None, 'tversky' or 'dice'")
        self.region = region
        if region == "dice":
            if region_alpha is not None or region_beta is not None:
                raise ValueError("FusedSegLoss: region='dice' is alpha = beta = 0.5; region_alpha / region_beta "
                                 "go with region='tversky'")
            region_alpha = region_beta = 0.5
        self.region_alpha = 0.3 if region_alpha is None else float(region_alpha)
        self.region_beta = 0.7 if region_beta is None else float(region_beta)
        self.region_smooth = float(region_smooth)
        self.region_weight = float(region_weight)
        if not (self.region_alpha >= 0.0 and self.region_beta >= 0.0 and
                0.0 < self.region_alpha + self.region_beta < math.inf):
            raise ValueError(f"FusedSegLoss: region_alpha {region_alpha} and region_beta {region_beta} must be "
                             "finite, >= 0 and not both 0")
        if not (math.isfinite(self.region_smooth) and self.region_smooth > 0.0):
            raise ValueError(f"FusedSegLoss: region_smooth {region_smooth} must be > 0")
        if not (math.isfinite(self.region_weight) and self.region_weight >= 0.0):
            raise ValueError(f"FusedSegLoss: region_weight {region_weight} is not a finite number >= 0")

    def extra_repr(self):
        s = (f"ignore_index={self.ignore_index}, weight={None if self.weight is None else self.weight.numel()}, "
             f"label_smoothing={self.label_smoothing}, ohem_thresh={self.ohem_thresh}, "
             f"ohem_min_kept={self.ohem_min_kept}")
        if self.focal_gamma > 0.0:
            s += f", focal_gamma={self.focal_gamma}"
        if self.region is not None:
            s += (f", region={self.region!r}, region_weight={self.region_weight}, region_alpha={self.region_alpha}, "
                  f"region_beta={self.region_beta}, region_smooth={self.region_smooth}")
        return s

    def has_terms(self):
        """True if a focal or region term is set: those run on dformer_amd.criterion, not on SegLossFn alone."""
        return self.focal_gamma > 0.0 or self.region is not None

    def region_options(self):
        """(alpha, beta, smooth) or None, for criterion.SegTermsFn."""
        return None if self.region is None else (self.region_alpha, self.region_beta, self.region_smooth)

    def fused_terms(self, logits_rows, B, h, w, label, weight):
        """The terms SegLossFn does not compute, on the fused kernels (dformer_amd.criterion is imported here, on
        first use): with focal_gamma > 0 the focal pixel term and the region term in one pass, otherwise
        region_weight * L_reg alone (the caller adds SegLossFn's pixel term)."""
        from .criterion import SegTermsFn
        return SegTermsFn.apply(logits_rows, B, h, w, label, self.ignore_index, weight, self.focal_gamma,
                                self.focal_gamma > 0.0, self.region_options(), self.region_weight)

    def check_classes(self, ncls, what):
        """A weight vector must match the width of the head it is applied to."""
        if self.weight is not None and self.weight.numel() != ncls:
            raise ValueError(f"FusedSegLoss: weight has {self.weight.numel()} entries, {what} has {ncls} output "
                             "channels")

    def kernel_options(self, device):
        """(weight on `device` or None, label_smoothing, ohem_thresh or None, ohem_min_kept) for SegLossFn."""
        w = self.weight
        if w is not None and w.device != device:
            w = w.to(device)
        return w, self.label_smoothing, self.ohem_thresh, self.ohem_min_kept

    @torch.no_grad()
    def mined_target(self, pred, target):
        """target with the mined-out pixels set to ignore_index (loss_opr.py:157-185)."""
        if self.ohem_thresh is None:
            return target
        valid = target != self.ignore_index
        num_valid = int(valid.sum())
        if self.ohem_min_kept == 0 or self.ohem_min_kept > num_valid:
            return target
        prob = F.softmax(pred.float(), dim=1).gather(1, (target * valid).unsqueeze(1)).squeeze(1)
        kth = prob[valid].sort().values[self.ohem_min_kept - 1]
        threshold = torch.clamp_min(kth, self.ohem_thresh)
        return target.masked_fill(~(valid & (prob <= threshold)), self.ignore_index)

    def forward(self, pred, target):
        """pred [B, C, H, W] full-resolution logits, target [B, H, W] int64 -> the scalar loss (any device)."""
        target = target.long()
        if self.weight is not None:
            self.check_classes(pred.shape[1], "pred")
        if self.has_terms():
            return self._forward_terms(pred, target)
        kept = self.mined_target(pred.detach(), target)
        per = F.cross_entropy(pred.float(), kept, weight=self.weight, reduction="none",
                              ignore_index=self.ignore_index, label_smoothing=self.label_smoothing)
        n = (kept != self.ignore_index).sum()
        return per.sum() / n.clamp_min(1).to(per.dtype)

    def _forward_terms(self, pred, target):
        """The definition with a focal or region term, in float32 (float64 if pred is)."""
        x = pred if pred.dtype == torch.float64 else pred.float()
        C = x.shape[1]
        w = torch.ones(C, dtype=x.dtype, device=x.device) if self.weight is None else self.weight.to(x.dtype)
        valid = target != self.ignore_index
        safe = (target * valid).unsqueeze(1)
        if self.focal_gamma > 0.0:
            p = F.softmax(x, dim=1)
            logq = F.log_softmax(x, dim=1).gather(1, safe).squeeze(1)
            # 1 - q as the sum of the other classes; the clamp keeps d(.)^gamma finite where it underflows to 0
            omq = (p.sum(1) - p.gather(1, safe).squeeze(1)).clamp_min(torch.finfo(x.dtype).tiny)
            per = w[safe.squeeze(1)] * omq.pow(self.focal_gamma) * -logq * valid
            loss = per.sum() / valid.sum().clamp_min(1).to(x.dtype)
        else:
            kept = self.mined_target(pred.detach(), target)
            per = F.cross_entropy(x, kept, weight=w, reduction="none", ignore_index=self.ignore_index,
                                  label_smoothing=self.label_smoothing)
            loss = per.sum() / (kept != self.ignore_index).sum().clamp_min(1).to(x.dtype)
        if self.region is not None:
            v = valid.unsqueeze(1).to(x.dtype)
            pv = F.softmax(x, dim=1) * v
            onehot = torch.zeros_like(pv).scatter_(1, safe, 1.0) * v
            TP, SP, SY = (pv * onehot).sum((2, 3)), pv.sum((2, 3)), onehot.sum((2, 3))
            a, b, s = self.region_alpha, self.region_beta, self.region_smooth
            T = (TP + s) / (TP + a * (SP - TP) + b * (SY - TP) + s)
            loss = loss + self.region_weight * ((w * (1.0 - T)).sum(1) / C).mean()
        return loss
