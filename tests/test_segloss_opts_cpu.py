"""losses.FusedSegLoss without a GPU: the direct call on full-resolution logits against an inline oracle
(class weights, label smoothing, hard example mining of utils/loss_opr.py:157-185), what EncoderDecoder
accepts and rejects, and the new C entry points' declarations."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dformer_hip.h")
NEW = ("dfm_seg_loss_opts_fwd", "dfm_seg_loss_opts_fwd_grad", "dfm_seg_loss_opts_bwd",
       "dfm_seg_loss_ohem_workspace", "dfm_seg_loss_ohem_relabel")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def cfg(ncls=40, **kw):
    c = Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=ncls, drop_path_rate=0.0,
            bn_eps=1e-3, bn_momentum=0.1, background=255)
    c.update(kw)
    return c


def oracle(pred, target, weight, eps, thresh, min_kept, ignore=255):
    """The issue's definition written out in float64: (loss, kept mask)."""
    C = pred.shape[1]
    logp = F.log_softmax(pred.double(), dim=1)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    valid = target != ignore
    y = (target * valid).unsqueeze(1)
    per = (1 - eps) * w[y.squeeze(1)] * -logp.gather(1, y).squeeze(1) + eps / C * (-logp * w.view(1, C, 1, 1)).sum(1)
    kept = valid
    n = int(valid.sum())
    if thresh is not None and 0 < min_kept <= n:
        p = logp.exp().gather(1, y).squeeze(1)
        kth = p[valid].sort().values[min_kept - 1]
        kept = valid & (p <= max(thresh, float(kth)))
    return (per * kept).sum() / max(int(kept.sum()), 1), kept


def inputs(C=7, B=2, H=9, W=11, frac_ignored=0.1):
    g = torch.Generator().manual_seed(C)
    pred = 3 * torch.randn(B, C, H, W, generator=g)
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < frac_ignored] = 255
    weight = 0.5 + 1.5 * torch.rand(C, generator=g)
    weight[C // 2] = 0.0
    return pred, target, weight


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ohem", [None, (0.01, 130), (0.6, 20), (0.6, 0), (0.6, 10 ** 6)])
def test_direct_call_matches_oracle(ohem, weighted, eps):
    from dformer_amd.losses import FusedSegLoss
    pred, target, weight = inputs()
    weight = weight if weighted else None
    thresh, k = ohem if ohem else (None, 0)
    crit = FusedSegLoss(255, weight, eps, ohem_thresh=thresh, ohem_min_kept=k)
    p = pred.clone().requires_grad_()
    loss = crit(p, target)
    ref, kept = oracle(pred, target, weight, eps, thresh, k)
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    n = int((target != 255).sum())
    if ohem == (0.01, 130):  # the k-th smallest probability is above the floor: exactly k kept (no ties here)
        assert int(kept.sum()) == 130 < n
    elif ohem == (0.6, 20):  # the floor is above it: everything at or under 0.6 is kept
        assert 20 < int(kept.sum()) < n
    else:                    # no mining: every valid pixel
        assert int(kept.sum()) == n
    assert torch.equal(crit.mined_target(pred, target) != 255, kept)
    loss.backward()          # the selection carries no gradient: pixels outside K get none
    assert torch.all(p.grad.abs().sum(1)[~kept] == 0)


def test_direct_call_all_ignored_and_denominator():
    from dformer_amd.losses import FusedSegLoss
    pred, target, weight = inputs()
    crit = FusedSegLoss(255, weight, 0.1, ohem_thresh=0.6, ohem_min_kept=5)
    p = pred.clone().requires_grad_()
    loss = crit(p, torch.full_like(target, 255))
    loss.backward()
    assert loss.item() == 0.0 and torch.all(p.grad == 0)
    # the mean divides by the pixel count, not the weight sum (nn.CrossEntropyLoss(reduction='mean') does)
    plain = FusedSegLoss(255, weight)(pred, target)
    per = F.cross_entropy(pred, target, weight=weight, reduction="none", ignore_index=255)
    assert abs(plain.item() - per[target != 255].mean().item()) < 1e-6 * plain.item()
    assert abs(plain.item() - F.cross_entropy(pred, target, weight=weight, ignore_index=255).item()) > 1e-3


def test_constructor_rejects_bad_options():
    from dformer_amd.losses import FusedSegLoss
    for eps in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            FusedSegLoss(255, None, eps)
    with pytest.raises(ValueError):
        FusedSegLoss(255, [1.0, -0.5, 1.0])
    with pytest.raises(ValueError):
        FusedSegLoss(255, torch.ones(65))
    with pytest.raises(ValueError):
        FusedSegLoss(255, None, 0.0, ohem_thresh=1.5)
    with pytest.raises(ValueError):
        FusedSegLoss(255, None, 0.0, ohem_thresh=0.5, ohem_min_kept=-1)


def test_segmentor_accepts_and_checks_the_criterion():
    from dformer_amd.losses import FusedSegLoss
    from dformer_amd.segmentor import EncoderDecoder
    w40 = torch.linspace(0.5, 2.0, 40)
    crit = FusedSegLoss(255, w40, 0.1, ohem_thresh=0.7, ohem_min_kept=1000)
    m = EncoderDecoder(cfg=cfg(), criterion=crit)
    assert m.criterion is crit
    # the criterion adds nothing to the checkpoint: the state_dict keeps the reference's keys
    assert not any(k.startswith("criterion") for k in m.state_dict())
    assert EncoderDecoder(cfg=cfg(aux_rate=0.4), criterion=crit).aux_head.num_classes == 40
    with pytest.raises(ValueError, match="ignore_index"):
        EncoderDecoder(cfg=cfg(), criterion=FusedSegLoss(0, w40))
    with pytest.raises(ValueError, match="decode head"):
        EncoderDecoder(cfg=cfg(), criterion=FusedSegLoss(255, torch.ones(37)))
    # the ham aux head is 40 wide whatever cfg.num_classes says (builder.py:143)
    EncoderDecoder(cfg=cfg(37), criterion=FusedSegLoss(255, torch.ones(37)))
    with pytest.raises(ValueError, match="aux head"):
        EncoderDecoder(cfg=cfg(37, aux_rate=0.4), criterion=FusedSegLoss(255, torch.ones(37)))
    EncoderDecoder(cfg=cfg(37, aux_rate=0.4), criterion=FusedSegLoss(255, None, 0.1))
    # nn.CrossEntropyLoss with options stays rejected, and the message names the replacement
    with pytest.raises(NotImplementedError, match="dformer_amd.losses.FusedSegLoss"):
        EncoderDecoder(cfg=cfg(), criterion=torch.nn.CrossEntropyLoss(weight=w40, reduction="none",
                                                                      ignore_index=255))


def test_new_symbols_declared_bound_and_exported():
    from dformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert _lib.lib.dfm_abi_version() == 13 == _lib.ABI_VERSION  # new symbols, no layout change
    for name in NEW:
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1]), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    raw = open(HEADER).read()
    assert "builder.py:230" in raw and "loss_opr.py:137-187" in raw
    assert _lib.lib.dfm_seg_loss_ohem_workspace(16, 480, 640) > 0


@pytest.mark.parametrize("name", [n for n in NEW if not n.endswith("workspace")])
def test_unknown_dtype_is_rejected_first(name):
    from dformer_amd import _lib
    res, argtypes = _lib._SIGS[name]
    assert res is ctypes.c_int and argtypes[0] is ctypes.c_int
    args = [0.0 if t is ctypes.c_float else 0 if t in (ctypes.c_int, ctypes.c_long) else None for t in argtypes]
    args[0] = 7
    st = getattr(_lib.lib, name)(*args)
    err = _lib.lib.dfm_last_error().decode()
    assert st == -2, (name, st, err)
    assert err.startswith(name + ": ") and "unsupported dtype 7" in err, err


def test_bad_arguments_fail_before_any_launch():
    """ncls <= 64, label_smoothing in [0, 1), thresh in [0, 1]: rejected with the function's name."""
    from dformer_amd import _lib
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: validation fails first
    L = _lib.lib
    st = L.dfm_seg_loss_opts_fwd(0, 1, 2, 2, 65, fake, 8, 8, fake, 255, None, 0.0, fake, fake, None)
    assert st == -1 and L.dfm_last_error().startswith(b"dfm_seg_loss_opts_fwd: ")
    st = L.dfm_seg_loss_opts_bwd(0, 1, 2, 2, 8, fake, 8, 8, fake, 255, None, 1.0, fake, None, fake, fake, None)
    assert st == -1 and b"dfm_seg_loss_opts_bwd: label_smoothing" in L.dfm_last_error()
    st = L.dfm_seg_loss_opts_fwd_grad(0, 1, 2, 2, 8, fake, 6, 6, fake, 255, None, 0.0, fake, fake, None)
    assert st == -1 and L.dfm_last_error().startswith(b"dfm_seg_loss_opts_fwd_grad: ")  # x3 has no fused tiles
    st = L.dfm_seg_loss_ohem_relabel(0, 1, 2, 2, 8, fake, 8, 8, fake, 255, 1.5, 10, fake, fake, fake, fake, None)
    assert st == -1 and L.dfm_last_error().startswith(b"dfm_seg_loss_ohem_relabel: thresh")
    st = L.dfm_seg_loss_ohem_relabel(0, 1, 2, 2, 65, fake, 8, 8, fake, 255, 0.5, 10, fake, fake, fake, fake, None)
    assert st == -1 and L.dfm_last_error().startswith(b"dfm_seg_loss_ohem_relabel: ")
