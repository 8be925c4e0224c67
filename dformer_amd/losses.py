"""Criteria of the fused segmentation loss.

FusedSegLoss is the criterion EncoderDecoder takes when the plain CrossEntropyLoss of utils/train.py:189-194
is not enough: class weights and label smoothing (the nn.CrossEntropyLoss arguments, builder.py:230) and
online hard example mining (utils/loss_opr.py:137-187, ProbOhemCrossEntropy2d). Inside the segmentor the
options go to the fused HIP loss (decoders.SegLossFn): the full-resolution logits are never materialised.
Called directly on full-resolution logits, forward() below is the same definition in plain torch ops.

Not taken over from ProbOhemCrossEntropy2d: its `use_weight` table of 19 Cityscapes class weights (pass
`weight=`) and `down_ratio` (its own forward never reads it).
"""
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
    """

    def __init__(self, ignore_index=255, weight=None, label_smoothing=0.0, ohem_thresh=None, ohem_min_kept=0):
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

    def extra_repr(self):
        return (f"ignore_index={self.ignore_index}, weight={None if self.weight is None else self.weight.numel()}, "
                f"label_smoothing={self.label_smoothing}, ohem_thresh={self.ohem_thresh}, "
                f"ohem_min_kept={self.ohem_min_kept}")

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
        kept = self.mined_target(pred.detach(), target)
        per = F.cross_entropy(pred.float(), kept, weight=self.weight, reduction="none",
                              ignore_index=self.ignore_index, label_smoothing=self.label_smoothing)
        n = (kept != self.ignore_index).sum()
        return per.sum() / n.clamp_min(1).to(per.dtype)
