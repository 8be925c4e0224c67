"""EncoderDecoder (models/builder.py:91-235): backbone + decode head + CE loss, on HIP kernels.

forward(rgb, modal_x, label) -> (loss, out) in training, out in eval, like the reference. The
backbone's `(outs, None)` tuple is indexed before the decode head (the reference HEAD passes the
tuple through and crashes, SURVEY.md §3.0 #2 — the intended upstream semantics are reproduced).
`out` is the full-resolution logits (bilinear, align_corners=False); during training it is only
materialised when `return_logits` is True (the loss itself is fused and never needs it).
With `decoder == "ham"` and a non-zero `cfg.aux_rate` an auxiliary FCNHead reads the stage-2 map and the
training loss is CE(main) + aux_rate * CE(aux) (builder.py:138-143, 204-207, 231-232); no eval path runs it.
`criterion` is the reference's plain CrossEntropyLoss or a losses.FusedSegLoss (class weights, label
smoothing, hard example mining, focal and Tversky / Dice terms; applied to the main and the aux loss, all on
the fused kernels).
`decoder == "UPernet"` builds UPerHead on all four maps (logits at 1/4 resolution) and always the aux head
with aux_rate 0.4 (builder.py:145-152).
"""
import torch
import torch.nn as nn

from . import kernels as K
from .decoders import (DecoderHead, FCNHead, FssLossFn, FssProtoSimFn, LightHamHead, SegLossFn, UPerHead,
                       _nhwc_rows)
from .encoder import DFormer_Base, DFormer_Large, DFormer_Small, DFormer_Tiny, get_DFormerTrav
from .functional import invalidate_weights
from .losses import FusedSegLoss

BACKBONES = {"DFormer-Tiny": (DFormer_Tiny, [32, 64, 128, 256]), "DFormer-Small": (DFormer_Small, [64, 128, 256, 512]),
             "DFormer-Base": (DFormer_Base, [64, 128, 256, 512]), "DFormer-Large": (DFormer_Large, [96, 192, 288, 576]),
             # builder.py:109-111: modal_x is a laser scan [B, 1, 360], expanded to the depth plane
             "DFormerTrav-Base": (get_DFormerTrav, [64, 128, 256, 512])}


def _check_criterion(criterion, ignore_index):
    """The loss is the fused kernel of builder.py:203,230: unweighted CrossEntropyLoss(reduction='none',
    ignore_index=cfg.background) followed by the mean over valid pixels (what train.py:189-194
    passes), or a losses.FusedSegLoss with the same ignore_index (class weights, label smoothing, hard
    example mining on the fused kernels). Anything else would be silently ignored, so it is rejected."""
    if criterion is None:
        return
    if isinstance(criterion, FusedSegLoss):
        if criterion.ignore_index != ignore_index:
            raise ValueError(f"EncoderDecoder: FusedSegLoss(ignore_index={criterion.ignore_index}) does not match "
                             f"cfg.background = {ignore_index}")
        return
    ok = (isinstance(criterion, nn.CrossEntropyLoss) and criterion.weight is None and
          criterion.reduction == "none" and criterion.ignore_index == ignore_index and
          float(getattr(criterion, "label_smoothing", 0.0)) == 0.0)
    if not ok:
        raise NotImplementedError(
            f"EncoderDecoder: the fused segmentation loss implements CrossEntropyLoss(reduction='none', "
            f"ignore_index={ignore_index}) without class weights or label smoothing (utils/train.py:189-194); "
            f"for class weights, label smoothing or hard example mining pass a "
            f"dformer_amd.losses.FusedSegLoss; got {criterion!r}")


def _aux_rate(cfg):
    """cfg.aux_rate, 0 when the config has no such name (a dict-backed config raises KeyError)."""
    try:
        rate = getattr(cfg, "aux_rate")
    except (AttributeError, KeyError):
        return 0
    return 0 if rate is None else rate


class EncoderDecoder(nn.Module):
    def __init__(self, cfg=None, criterion=None, norm_layer=nn.BatchNorm2d, syncbn=False):
        super().__init__()
        self.cfg = cfg
        self.norm_layer = norm_layer
        backbone, self.channels = BACKBONES[cfg.backbone]
        norm_cfg = dict(type="SyncBN" if syncbn else "BN", requires_grad=True)
        dpr = cfg.drop_path_rate if getattr(cfg, "drop_path_rate", None) is not None else 0.1
        self.encoder_backbone = backbone(drop_path_rate=dpr, norm_cfg=norm_cfg)
        bn_eps = getattr(cfg, "bn_eps", 1e-3)
        bn_mom = getattr(cfg, "bn_momentum", 0.1)
        if cfg.decoder == "MLPDecoder":
            self.decode_head = DecoderHead(in_channels=self.channels, num_classes=cfg.num_classes,
                                           norm_layer=norm_layer, embed_dim=cfg.decoder_embed_dim, bn_eps=bn_eps,
                                           bn_momentum=bn_mom, syncbn=syncbn)
        elif cfg.decoder == "ham":
            self.decode_head = LightHamHead(in_channels=self.channels[1:], num_classes=cfg.num_classes,
                                            in_index=[1, 2, 3], norm_cfg=norm_cfg, channels=cfg.decoder_embed_dim,
                                            bn_eps=bn_eps, bn_momentum=bn_mom)
        elif cfg.decoder == "UPernet":
            self.decode_head = UPerHead(in_channels=self.channels, num_classes=cfg.num_classes, norm_layer=norm_layer,
                                        channels=512, bn_eps=bn_eps, bn_momentum=bn_mom, syncbn=syncbn)
        else:
            raise NotImplementedError(f"decoder {cfg.decoder!r} is outside the hot path (SURVEY.md §2)")
        self.aux_head = None
        self.aux_rate = 0
        if cfg.decoder == "UPernet":
            # builder.py:149-152: the aux head and its rate are hard-coded, whatever cfg.aux_rate says
            self.aux_index = 2
            self.aux_rate = 0.4
            self.aux_head = FCNHead(self.channels[2], cfg.num_classes, norm_layer=norm_layer, bn_eps=bn_eps,
                                    bn_momentum=bn_mom, syncbn=syncbn)
        elif cfg.decoder == "ham" and _aux_rate(cfg) != 0:
            # builder.py:138-143: FCNHead(self.channels[2], cfg.num_classes, ...) binds cfg.num_classes to
            # the hidden width `channels`; the head's own num_classes stays 40 whatever the config says
            self.aux_index = 2
            self.aux_rate = _aux_rate(cfg)
            self.aux_head = FCNHead(self.channels[2], cfg.num_classes, norm_layer=norm_layer, bn_eps=bn_eps,
                                    bn_momentum=bn_mom, syncbn=syncbn)
        _check_criterion(criterion, getattr(cfg, "background", 255))
        if isinstance(criterion, FusedSegLoss):  # one weight per output channel of every head it is applied to
            criterion.check_classes(cfg.num_classes, "the decode head")
            if self.aux_head is not None:
                criterion.check_classes(self.aux_head.num_classes, "the aux head")
        self.criterion = criterion
        self.ignore_index = getattr(cfg, "background", 255)
        self.return_logits = True
        self.keep_episode = False  # meta_forward leaves proto / prob / foot / count in self.last_episode (tests)
        self.last_episode = None

    def set_compute_dtype(self, dtype):
        self.encoder_backbone.compute_dtype = dtype
        return self

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        invalidate_weights()
        return r

    def _low_logits(self, rgb, modal_x, with_aux=False):
        """The decode head's low-resolution logits; with_aux (training with an aux head) also the aux
        head's (builder.py:204-206). Every eval path leaves the aux head out: the reference computes its
        logits there and throws them away."""
        outs = self.encoder_backbone(rgb, modal_x)
        if isinstance(outs, tuple):  # DFormer returns (outs, None), DFormerTrav the list itself
            outs = outs[0]
        K.TAG = "decoder"
        low = self.decode_head.forward(outs)
        if not with_aux:
            return low
        K.TAG = "aux"
        return low, self.aux_head(outs[self.aux_index])

    def _low_rows(self, rgb, modal_x):
        """The low-res logits as NHWC rows: ([B*h*w, ncls], (B, h, w))."""
        return _nhwc_rows(self._low_logits(rgb, modal_x))

    def _upsample(self, low, size):
        rows, (B, h, w) = _nhwc_rows(low)
        up = K.bilinear(rows.contiguous(), (h, w), tuple(size), B)
        return up.view(B, size[0], size[1], -1).permute(0, 3, 1, 2)

    def encode_decode(self, rgb, modal_x):
        low = self._low_logits(rgb, modal_x)
        return self._upsample(low, rgb.shape[-2:])

    @torch.no_grad()
    def predict(self, rgb, modal_x):
        """The class map of the eval forward, uint8 [B, H, W]: forward(rgb, modal_x).argmax(1) without the
        full-resolution logits (one fused upsample + argmax kernel over the low-res logits)."""
        rows, (B, h, w) = self._low_rows(rgb, modal_x)
        K.TAG = "eval"
        return K.seg_predict(rows, B, h, w, rows.shape[1], tuple(rgb.shape[-2:]))

    def forward(self, rgb, modal_x=None, label=None):
        if label is None:
            return self._upsample(self._low_logits(rgb, modal_x), rgb.shape[-2:])
        aux = None
        if self.aux_head is not None:
            low, aux = self._low_logits(rgb, modal_x, with_aux=True)
        else:
            low = self._low_logits(rgb, modal_x)
        rows, (B, h, w) = _nhwc_rows(low)
        K.TAG = "loss"
        # a FusedSegLoss criterion's options apply to both heads (builder.py:230-232 calls the one criterion
        # on each); the aux head is mined on its own probabilities
        opts = self.criterion.kernel_options(rows.device) if isinstance(self.criterion, FusedSegLoss) else ()
        if opts and self.criterion.has_terms():
            head_loss = self._terms_loss  # a focal or region term: dformer_amd.criterion, loaded on first use
        else:
            def head_loss(r, B, h, w, label, opts):
                return SegLossFn.apply(r, B, h, w, label, self.ignore_index, *opts)
        loss = head_loss(rows.contiguous(), B, h, w, label.long(), opts)
        if aux is not None:  # builder.py:231-232: + aux_rate * CE(up(aux)) over the same valid pixels
            arows, (B, ah, aw) = _nhwc_rows(aux)
            loss = loss + self.aux_rate * head_loss(arows.contiguous(), B, ah, aw, label.long(), opts)
        out = self._upsample(low.detach(), rgb.shape[-2:]) if self.return_logits else low
        return loss, out

    def _terms_loss(self, rows, B, h, w, label, opts):
        """One head's loss under a FusedSegLoss with a focal or region term. focal_gamma > 0: the new function
        alone computes the pixel and the region term in one pass; region only: SegLossFn as always (weights,
        smoothing, mining) plus the region term on the original labels."""
        crit = self.criterion
        terms = crit.fused_terms(rows, B, h, w, label, opts[0])
        if crit.focal_gamma > 0.0:
            return terms
        return SegLossFn.apply(rows, B, h, w, label, self.ignore_index, *opts) + terms

    # ------------------------------------------------------------------ few-shot episodes (builder.py:210-320)
    def encode(self, rgb, modal_x):
        """builder.py:210-211: the backbone's four maps (DFormer's (outs, None) tuple is indexed)."""
        outs = self.encoder_backbone(rgb, modal_x)
        return outs[0] if isinstance(outs, tuple) else outs

    def decode(self, x, rgb):
        """builder.py:213-222: the decode head on the maps x, upsampled to rgb's size (with an aux head, the
        pair (out, aux) like the reference)."""
        K.TAG = "decoder"
        out = self._upsample(self.decode_head.forward(x), rgb.shape[-2:])
        if self.aux_head is None:
            return out
        K.TAG = "aux"
        return out, self._upsample(self.aux_head(x[self.aux_index]), rgb.shape[-2:])

    def _fss_config(self):
        """(alpha, temperature) of the episode head, after the checks meta_forward makes up front."""
        if self.cfg.num_classes != 2:
            raise NotImplementedError(f"meta_forward: the reference stacks exactly [bg, fg] (builder.py:296); "
                                      f"cfg.num_classes = {self.cfg.num_classes} is not 2")
        if self.aux_head is not None:
            raise NotImplementedError("meta_forward: with an aux head the reference's decode returns a tuple that "
                                      "alpha * logits cannot take (builder.py:218-221, 303); set cfg.aux_rate = 0")
        vals = []
        for name in ("alpha", "temperature"):
            try:
                v = getattr(self.cfg, name)
            except (AttributeError, KeyError):
                v = None
            if v is None:
                raise ValueError(f"meta_forward: cfg.{name} is missing (local_configs/Trav/DFormer_Base.py sets "
                                 "alpha = 0.5, temperature = 1)")
            vals.append(float(v))
        if not vals[1] > 0.0:
            raise ValueError(f"meta_forward: cfg.temperature = {vals[1]} must be positive")
        return tuple(vals)

    def meta_forward(self, s_rgb, s_depth, s_mask, q_rgb, q_depth, q_gt=None):
        """builder.py:237-310, one few-shot episode batch: s_rgb [B, S, 3, H, W], s_depth [B, S, 1, N] (whatever
        the backbone's modal_x is per image), s_mask [B, S, H, W] (1 = foreground, 0 = background, anything
        else, 255 included, in neither prototype), q_rgb [B, 3, H, W], q_depth [B, 1, N], q_gt [B, H, W].
        Returns (loss, fused_logits [B, 2, H, W]) with q_gt, fused_logits without; with return_logits False the
        training call returns the decode head's low-res logits in place of fused_logits, as forward does.
        The ignore label of q_gt is 255, hard-coded as in the reference (builder.py:307), not cfg.background.
        One encoder pass over the B*S + B images; the prototype pooling, the cosine branch and the loss run on
        stage-3 sized tensors; nothing is read back to the host."""
        alpha, temperature = self._fss_config()
        if isinstance(self.criterion, FusedSegLoss) and self.criterion.has_terms():
            raise NotImplementedError("meta_forward: the episode loss has its own kernels and takes no focal or "
                                      "region term; they would be silently dropped (use a FusedSegLoss without "
                                      "focal_gamma / region)")
        if s_rgb.dim() != 5 or s_mask.dim() != 4 or tuple(s_mask.shape[:2]) != tuple(s_rgb.shape[:2]):
            raise ValueError(f"meta_forward: s_rgb {tuple(s_rgb.shape)} / s_mask {tuple(s_mask.shape)} are not "
                             "[B, S, 3, H, W] / [B, S, H, W]")
        B, S = s_rgb.shape[:2]
        H, W = s_rgb.shape[-2:]
        if q_rgb.shape[0] != B or tuple(q_rgb.shape[-2:]) != (H, W) or tuple(s_mask.shape[-2:]) != (H, W):
            raise ValueError(f"meta_forward: q_rgb {tuple(q_rgb.shape)} / s_mask {tuple(s_mask.shape)} do not match "
                             f"{B} episodes of {H} x {W} images")
        if q_gt is not None and tuple(q_gt.shape) != (B, H, W):
            raise ValueError(f"meta_forward: q_gt {tuple(q_gt.shape)} is not [{B}, {H}, {W}]")
        all_rgb = torch.cat([s_rgb.reshape(B * S, -1, H, W), q_rgb.reshape(B, -1, H, W)], 0)
        all_x = torch.cat([s_depth.reshape(B * S, *s_depth.shape[2:]), q_depth.reshape(B, *q_depth.shape[1:])], 0)
        feats = self.encode(all_rgb, all_x)
        K.TAG = "fss"
        hs, ws = feats[-1].shape[-2:]
        foot, count = K.fss_mask_footprint(s_mask.reshape(B * S, H, W).long().contiguous(), (hs, ws))
        q3, prob, proto = FssProtoSimFn.apply(feats[-1], foot, count, B, S, temperature)
        K.TAG = "decoder"
        low = self.decode_head.forward([x[B * S:] for x in feats[:-1]] + [q3])
        rows, (_, h, w) = _nhwc_rows(low)
        K.TAG = "fss"
        if self.keep_episode:
            self.last_episode = dict(proto=proto.detach(), prob=prob.detach().view(B, hs, ws, 2), foot=foot, count=count)

        def fused():
            out = K.fss_fuse(rows.detach(), B, h, w, prob.detach(), hs, ws, (H, W), alpha)
            return out.view(B, H, W, 2).permute(0, 3, 1, 2)

        if q_gt is None:
            return fused()
        loss = FssLossFn.apply(rows, prob, B, h, w, hs, ws, q_gt.long(), alpha)
        return loss, (fused() if self.return_logits else low)
