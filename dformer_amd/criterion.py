"""The focal and Tversky / Dice terms of losses.FusedSegLoss on the GPU, fused with the bilinear upsample of a
head's low-resolution logits: the full-resolution logits are never materialised.

    loss = SegTermsFn.apply(logits_rows, B, h, w, label, ignore, weight, focal_gamma, has_pixel, region,
                            region_weight)

This module binds libdformer_criterion.so (include/dformer_criterion.h), a library of its own: losses.py
imports it on the first use of focal_gamma or region, so `import dformer_amd.segmentor` and a training run with
the default criterion map the model library alone. There is no torch fallback: a missing library is an
ImportError. The model library's launch tracer does not see this library's launches; the census still gets one
untimed entry per call under the caller's tag.
"""
import ctypes
import os

import torch

from . import kernels as K
from ._lib import dtype_code, ptr, stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdformer_criterion.so")

MAX_CLASSES, MAX_DIM, MAX_BATCH = 64, 16384, 65535  # DFC_MAX_CLASSES, DFC_MAX_DIM, DFC_MAX_BATCH
c_int, c_float, c_size_t, P = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p


class TermsDesc(ctypes.Structure):
    """DfcTermsDesc."""
    _fields_ = [("gamma", c_float), ("alpha", c_float), ("beta", c_float), ("smooth", c_float),
                ("has_pixel", c_int), ("has_region", c_int)]


_DESC = ctypes.POINTER(TermsDesc)
# name -> (restype, argtypes)
_SIGS = {
    "dfc_last_error": (ctypes.c_char_p, []),
    "dfc_abi_version": (c_int, []),
    "dfc_seg_terms_workspace": (c_size_t, [c_int] * 6),
    "dfc_seg_terms_fwd": (c_int, [c_int] * 5 + [P, c_int, c_int, P, c_int, P, _DESC, P, P, P, P]),
    "dfc_seg_terms_bwd": (c_int, [c_int] * 5 + [P, c_int, c_int, P, c_int, P, _DESC, P, P, P, c_float, P, P]),
}

ABI_VERSION = 1  # the dfc_abi_version() TermsDesc and _SIGS were written for


def check_abi(lib):
    got = lib.dfc_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"dformer_amd.criterion: {LIB_PATH} has ABI version {got}, these bindings expect "
                          f"{ABI_VERSION}; rebuild it from this tree's csrc")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"dformer_amd.criterion: native library missing at {LIB_PATH}; run "
                          f"`python -c 'import __graft_entry__ as g; g.build()'` (make -C dformer_amd/csrc)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    check_abi(lib)
    return lib


lib = _load()


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {lib.dfc_last_error().decode()}")


def make_desc(focal_gamma=0.0, has_pixel=True, region=None):
    """region: None or (alpha, beta, smooth)."""
    alpha, beta, smooth = region if region is not None else (0.0, 0.0, 0.0)
    return TermsDesc(float(focal_gamma), float(alpha), float(beta), float(smooth), int(bool(has_pixel)),
                     int(region is not None))


def _args(what, logits, B, h, w, label, weight):
    ncls = logits.shape[-1]
    if logits.dim() != 2 or not logits.is_cuda or not logits.is_contiguous() or logits.shape[0] != B * h * w:
        raise ValueError(f"{what}: logits {tuple(logits.shape)} are not contiguous device rows [{B}*{h}*{w}, ncls]")
    if label.dtype != torch.int64 or not label.is_contiguous() or label.dim() != 3 or label.shape[0] != B or \
            label.device != logits.device:
        raise ValueError(f"{what}: label {tuple(label.shape)} {label.dtype} is not contiguous int64 [{B}, H, W] on "
                         f"{logits.device}")
    if weight is not None and (weight.dtype != torch.float32 or not weight.is_contiguous() or
                               weight.numel() != ncls or weight.device != logits.device):
        raise ValueError(f"{what}: weight {tuple(weight.shape)} {weight.dtype} on {weight.device} is not contiguous "
                         f"float32 [{ncls}] on {logits.device}")
    return ncls, label.shape[1], label.shape[2]


def _account(nbytes):
    if K.ACCOUNT is not None:  # no kernel handle: the model library's tracer does not see these launches
        K.ACCOUNT.append(((), 0.0, float(nbytes), "bf16", K.TAG))


def seg_terms_fwd(logits, B, h, w, label, desc, weight=None, ignore=255):
    """-> (stats float32 [B, ncls, 3] = (TP, SP, SY), out float32 [3] = (pixel-term sum, valid count, L_reg))."""
    ncls, H, W = _args("seg_terms_fwd", logits, B, h, w, label, weight)
    dev = logits.device
    stats = torch.empty(B, ncls, 3, device=dev, dtype=torch.float32)
    out = torch.empty(3, device=dev, dtype=torch.float32)
    # block partials, about 1/128 of the full-resolution logits: a buffer of this call (the allocator reuses it
    # in stream order), not the model library's shared scratch with its 1 MiB floor
    ws = torch.empty(lib.dfc_seg_terms_workspace(B, h, w, ncls, H, W), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(lib.dfc_seg_terms_fwd(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                    ptr(weight), desc, ptr(ws), ptr(stats), ptr(out), stream()),
              "dfc_seg_terms_fwd")
    _account(logits.numel() * logits.element_size() + label.numel() * 8)
    return stats, out


def seg_terms_bwd(logits, B, h, w, label, desc, stats, out, gscale=None, region_weight=1.0, weight=None,
                  ignore=255):
    """-> gscale * d(out[0] / max(out[1], 1) + region_weight * out[2]) / d logits, in the logits' dtype."""
    ncls, H, W = _args("seg_terms_bwd", logits, B, h, w, label, weight)
    if tuple(stats.shape) != (B, ncls, 3) or stats.dtype != torch.float32 or not stats.is_contiguous() or \
            out.numel() != 3 or out.dtype != torch.float32:
        raise ValueError(f"seg_terms_bwd: stats {tuple(stats.shape)} / out {tuple(out.shape)} are not the forward's")
    if gscale is not None and (gscale.dtype != torch.float32 or gscale.numel() != 1 or
                               gscale.device != logits.device):
        raise ValueError("seg_terms_bwd: gscale is not a float32 [1] on the logits' device")
    dl = torch.empty_like(logits)
    with torch.cuda.device(logits.device):
        check(lib.dfc_seg_terms_bwd(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                    ptr(weight), desc, ptr(stats), ptr(out), ptr(gscale), float(region_weight),
                                    ptr(dl), stream()), "dfc_seg_terms_bwd")
    _account(2 * logits.numel() * logits.element_size() + label.numel() * 8)
    return dl


class SegTermsFn(torch.autograd.Function):
    """[has_pixel] sum_i v_i w[y_i] (1 - p_i)^gamma (-log p_i) / max(sum_i v_i, 1) + region_weight * L_reg on the
    bilinear upsample of logits_rows [B*h*w, ncls] (losses.FusedSegLoss states both terms). region is None or
    (alpha, beta, smooth); weight float32 [ncls] on the device or None. The backward returns the gradient in
    the logits' dtype; the upstream gradient (with a loss scale) stays on the device."""

    @staticmethod
    def forward(ctx, logits_rows, B, h, w, label, ignore, weight, focal_gamma, has_pixel, region, region_weight):
        if not has_pixel and region is None:
            raise ValueError("SegTermsFn: neither the pixel term nor a region term is asked for")
        label = label.contiguous()
        desc = make_desc(focal_gamma, has_pixel, region)
        stats, out = seg_terms_fwd(logits_rows, B, h, w, label, desc, weight, ignore)
        ctx.save_for_backward(logits_rows, label, stats, out, *([weight] if weight is not None else []))
        ctx.meta = (B, h, w, ignore, desc, float(region_weight))
        loss = out[2] * float(region_weight) if region is not None else None
        if has_pixel:
            pix = out[0] / out[1].clamp_min(1.0)
            loss = pix if loss is None else pix + loss
        return loss

    @staticmethod
    def backward(ctx, g):
        K.TAG = "loss.bwd"
        B, h, w, ignore, desc, region_weight = ctx.meta
        logits_rows, label, stats, out = ctx.saved_tensors[:4]
        weight = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        gs = g.reshape(1).float().contiguous()
        dl = seg_terms_bwd(logits_rows, B, h, w, label, desc, stats, out, gs, region_weight, weight, ignore)
        return (dl,) + (None,) * 10
