"""Shared by tests/test_fss_*.py and oracle/golden_e2e.py: deterministic episode masks and a torch float64
restatement of the few-shot tail of meta_forward (models/builder.py:273-308) in its collapsed form
(DESIGN.md §6e). Nothing here touches the package under test or the reference."""
import numpy as np
import torch
import torch.nn.functional as F

import gen

E2E = dict(B=2, S=2, H=96, W=128, N=24, ncls=2, alpha=0.5, temperature=1.0)


def masks(name, n, H, W, seed=77, empty=()):
    """int64 [n, H, W]: per image a seeded rectangle of foreground (1), a band of 255 (two rows and two
    columns across the image) and background (0) elsewhere. i.i.d. noise masks would make both prototypes
    the mean feature. Images listed in `empty` get no foreground."""
    g = gen.rng(seed, name + "/masks")
    out = np.zeros((n, H, W), np.int64)
    for i in range(n):
        y0, x0 = int(g.integers(0, max(H // 2, 1))), int(g.integers(0, max(W // 2, 1)))
        hh, ww = int(g.integers(max(H // 4, 1), max(H // 2, 1) + 1)), int(g.integers(max(W // 4, 1), max(W // 2, 1) + 1))
        by, bx = int(g.integers(0, H)), int(g.integers(0, W))
        if i not in empty:
            out[i, y0:y0 + hh, x0:x0 + ww] = 1
        out[i, by:by + 2, :] = 255
        out[i, :, bx:bx + 2] = 255
    return out


def tap_matrix(n_in, n_out, dtype=torch.float64):
    """A [n_out, n_in]: row p holds the two bilinear taps (align_corners=False) of output index p, so that
    up(x) = A_y x A_x^T."""
    src = (torch.arange(n_out, dtype=dtype) + 0.5) * (n_in / n_out) - 0.5
    src = src.clamp_min(0.0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = src - i0.to(dtype)
    A = torch.zeros(n_out, n_in, dtype=dtype)
    A.scatter_add_(1, i0[:, None], (1.0 - l1)[:, None])
    A.scatter_add_(1, i1[:, None], l1[:, None])
    return A


def footprint64(mask, hs, ws):
    """(foot [n, 2, hs, ws], count [n, 2]) in float64: A_y^T [mask == k] A_x."""
    n, H, W = mask.shape
    Ay, Ax = tap_matrix(hs, H), tap_matrix(ws, W)
    ind = torch.stack([(mask == 0), (mask == 1)], 1).to(torch.float64)  # [n, 2, H, W]
    return Ay.t() @ ind @ Ax, ind.sum((2, 3))


def proto64(f, foot, count, B, S):
    """f [B*S, cells, C] -> proto [B, 2, C]: the masked average pool through the footprint, mean over shots.
    The denominator is float32(count + 1e-5) whatever the compute dtype: the reference's mask is `.float()`
    (builder.py:279-280, 314-316), so its `mask.sum() + 1e-5` is a float32 sum, in which the 1e-5 is rounded
    away above 256 pixels. The kernel adds in float32 too."""
    n, cells, C = f.shape
    den = (count.float() + 1e-5).double()
    p = torch.einsum("nkc,ncd->nkd", foot.reshape(n, 2, cells), f.double()) / den[..., None]
    return p.view(B, S, 2, C).mean(1)


def sim64(q, proto, temperature=1.0):
    """q [B, cells, C], proto [B, 2, C] -> (prob [B, cells, 2], cos [B, cells, 2]); norms clamped at 1e-8."""
    q = q.double()
    nq = q.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    npr = proto.norm(dim=-1).clamp_min(1e-8)
    cos = torch.einsum("bnc,bkc->bnk", q, proto) / (nq * npr[:, None, :])
    return torch.softmax(20.0 * cos / temperature, -1), cos


def up64(x, size):
    """x [B, h, w, C] -> [B, H, W, C] through the tap matrices."""
    Ay, Ax = tap_matrix(x.shape[1], size[0]), tap_matrix(x.shape[2], size[1])
    return torch.einsum("yh,bhwc,xw->byxc", Ay, x.double(), Ax)


def fused64(low, prob, size, alpha):
    """alpha up(low) + (1 - alpha) up(prob): low [B, h, w, 2], prob [B, hs, ws, 2] -> [B, H, W, 2]."""
    return alpha * up64(low, size) + (1.0 - alpha) * up64(prob, size)


def loss64(fused, label):
    """CE over the pixels labelled 0 / 1, mean; 0 when none is."""
    valid = (label == 0) | (label == 1)
    if not valid.any():
        return fused.sum() * 0.0
    return F.cross_entropy(fused[valid], label[valid].long())


def tail64(f_sup, f_qry, low, mask, label, B, S, alpha, temperature):
    """The collapsed few-shot tail in float64: f_sup [B*S, hs, ws, C], f_qry [B, hs, ws, C], low [B, h, w, 2],
    mask [B*S, H, W], label [B, H, W] -> dict(proto, prob, fused, loss)."""
    n, hs, ws, C = f_sup.shape
    foot, count = footprint64(mask, hs, ws)
    proto = proto64(f_sup.reshape(n, hs * ws, C), foot, count, B, S)
    prob, _ = sim64(f_qry.reshape(B, hs * ws, C), proto, temperature)
    prob = prob.view(B, hs, ws, 2)
    fused = fused64(low, prob, mask.shape[-2:], alpha)
    return dict(proto=proto, prob=prob, fused=fused, loss=loss64(fused, label), foot=foot, count=count)
