"""Few-shot episodes without a GPU: the float64 restatement of the collapsed tail (fss_common) against the
reference's golden, the footprint identities, the header / binding agreement of the dfm_fss_* symbols and the
host logic of meta_forward's checks and fss_evaluate's batch handling."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fss_common as FC
from goldens import load, rel_err
from test_abi import declared


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _golden_tail(g, empty=()):
    B, S, H, W, N, seed, mseed = [int(v) for v in g["meta"]]
    f3 = torch.from_numpy(g["f3"]).permute(0, 2, 3, 1)  # [B*S + B, hs, ws, C]
    low = torch.from_numpy(g["low64"]).permute(0, 2, 3, 1)
    mask = torch.from_numpy(FC.masks("e2e_fss_small", B * S, H, W, seed=mseed, empty=empty))
    lab = torch.from_numpy(FC.masks("e2e_fss_small/q", B, H, W))
    return FC.tail64(f3[:B * S], f3[B * S:], low, mask, lab, B, S, FC.E2E["alpha"], FC.E2E["temperature"])


def test_collapsed_restatement_matches_the_reference():
    """The reference upsamples the stage-3 map to the image and multiplies by the mask (builder.py:312-317);
    the collapse weights the stage-3 rows by the mask's footprint instead. Both in float64: 1e-9."""
    g = load("e2e_fss_small")
    t = _golden_tail(g)
    e = {"proto": rel_err(t["proto"], g["proto"]), "prob": rel_err(t["prob"], g["prob"]),
         "loss": abs(t["loss"].item() - float(g["loss"])) / abs(float(g["loss"]))}
    print("collapsed float64 restatement vs the reference: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v < 1e-9 for v in e.values()), e


def test_golden_conditions():
    """What the generator searched for: the similarity branch is neither flat nor saturated, and swapping the
    prototypes moves the loss far beyond the gate."""
    g = load("e2e_fss_small")
    fg = g["prob"][..., 1].reshape(-1)
    assert fg.std() >= 0.05 and ((fg > 0.02) & (fg < 0.98)).mean() >= 0.5
    assert g["cond"][2] > 100 * 1e-4 and float(g["margin"]) > 0
    B, S, H, W, N, seed, mseed = [int(v) for v in g["meta"]]
    m = FC.masks("e2e_fss_small", B * S, H, W, seed=mseed)
    assert all((m[i] == 0).any() and (m[i] == 1).any() and (m[i] == 255).any() for i in range(B * S))
    # swapped prototypes through the restatement: the same sensitivity
    t = _golden_tail(g)
    f3 = torch.from_numpy(g["f3"]).permute(0, 2, 3, 1)
    prob_sw, _ = FC.sim64(f3[B * S:].reshape(B, -1, f3.shape[-1]), t["proto"].flip(1))
    fused = FC.fused64(torch.from_numpy(g["low64"]).permute(0, 2, 3, 1), prob_sw.view(t["prob"].shape), (H, W), 0.5)
    lab = torch.from_numpy(FC.masks("e2e_fss_small/q", B, H, W))
    moved = abs(FC.loss64(fused, lab).item() - float(g["loss"])) / abs(float(g["loss"]))
    assert abs(moved - g["cond"][2]) < 1e-6 * g["cond"][2] + 1e-9


@pytest.mark.parametrize("n,hs,ws,H,W", [(1, 1, 1, 1, 1), (2, 3, 4, 96, 128), (2, 3, 5, 50, 77), (1, 15, 20, 480, 640)])
def test_footprint_identities(n, hs, ws, H, W):
    """sum over the cells of foot = count (the taps of a pixel sum to 1), and the footprint is the adjoint of
    F.interpolate: <up(x), m> = <x, foot>."""
    mask = torch.from_numpy(FC.masks(f"id{H}", n, H, W, empty=(0,)))
    foot, count = FC.footprint64(mask, hs, ws)
    assert torch.equal(count, torch.stack([(mask == 0).sum((1, 2)), (mask == 1).sum((1, 2))], 1).double())
    assert (foot.sum((2, 3)) - count).abs().max() <= 1e-12 * max(count.max().item(), 1.0)
    assert count[0, 1] == 0 and torch.count_nonzero(foot[0, 1]) == 0
    x = torch.from_numpy(np.random.default_rng(H).standard_normal((n, 2, hs, ws)))
    up = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)
    ind = torch.stack([mask == 0, mask == 1], 1).double()
    lhs, rhs = (up * ind).sum().item(), (x * foot).sum().item()
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), 1.0)


def test_empty_class_restatement():
    g = load("e2e_fss_small")
    t = _golden_tail(g, empty=(1,))
    assert t["count"][1, 1] == 0
    # the features of this forward are the ones stored (train-mode BN sees the same images: masks do not enter it)
    assert rel_err(t["proto"], g["proto_empty"]) < 1e-9 and rel_err(t["prob"], g["prob_empty"]) < 1e-9
    assert abs(t["loss"].item() - float(g["loss_empty"])) < 1e-9 * abs(float(g["loss_empty"]))


def test_fss_symbols_in_header_and_bindings():
    from dformer_amd import _lib
    d = declared()
    fss = sorted(n for n in d if n.startswith("dfm_fss_"))
    assert fss == sorted(n for n in _lib._SIGS if n.startswith("dfm_fss_")) and len(fss) == 12
    for n in fss:
        assert len(_lib._SIGS[n][1]) == d[n] and hasattr(_lib.lib, n), n
    assert _lib.lib.dfm_abi_version() == 13
    # validation happens on the host, before any launch
    assert _lib.lib.dfm_fss_footprint_workspace(1, 4, 4, 2, 2) == 0  # not an upsampling
    assert _lib.lib.dfm_fss_footprint_workspace(2, 3, 4, 96, 128) >= 2 * 2 * 96 * 4 * 4
    assert _lib.lib.dfm_fss_loss_fwd(7, *([0] * 3), None, 0, 0, 0, None, 0, 0, None, 0.0, None, None, None, None) == -2
    assert _lib.lib.dfm_fss_mask_footprint(1, 3, 4, 2, 2, *([None] * 5)) == -1


@pytest.mark.parametrize("name", ["dfm_fss_proto_pool_fwd", "dfm_fss_proto_pool_bwd", "dfm_fss_sim_fwd", "dfm_fss_sim_bwd",
                                  "dfm_fss_loss_fwd", "dfm_fss_loss_bwd", "dfm_fss_fuse_fwd"])
def test_fss_unknown_dtype_is_rejected_first(name):
    """The rule of tests/test_abi.py for the entry points that take a dtype code (their first argument)."""
    import ctypes
    from dformer_amd import _lib
    res, argtypes = _lib._SIGS[name]
    assert res is ctypes.c_int and argtypes[0] is ctypes.c_int
    args = [0.0 if t in (ctypes.c_float, ctypes.c_double) else
            0 if t in (ctypes.c_int, ctypes.c_long, ctypes.c_size_t) else None for t in argtypes]
    args[0] = 7
    st = getattr(_lib.lib, name)(*args)
    err = _lib.lib.dfm_last_error().decode()
    assert st == -2 and err.startswith(name + ": ") and "unsupported dtype 7" in err, (st, err)


class StubModel(torch.nn.Module):
    """meta_forward of a model that puts class q_depth[b, 0, 0] everywhere; records its calls."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def meta_forward(self, s_rgb, s_depth, s_mask, q_rgb, q_depth, q_gt=None):
        assert not self.training and q_gt is None
        self.calls.append(tuple(s_rgb.shape))
        B, _, H, W = q_rgb.shape
        cls = q_depth[:, 0, 0].long()
        out = torch.zeros(B, H, W, 2)
        out[torch.arange(B), :, :, cls] = 1.0
        return out.permute(0, 3, 1, 2)


def _stub_batch(B, cls, fn):
    gt = torch.zeros(B, 4, 6, dtype=torch.int64)
    gt[:, 0] = 255
    gt[:, 2:] = 1
    return dict(s_img=torch.zeros(B, 2, 3, 4, 6), s_depth=torch.zeros(B, 2, 1, 5), s_gt=torch.zeros(B, 2, 4, 6),
                q_img=torch.zeros(B, 3, 4, 6), q_depth=torch.full((B, 1, 5), float(cls)), q_gt=gt, fn=fn)


def test_fss_evaluate_batch_handling(monkeypatch):
    from dformer_amd import evaluate as Ev
    seen = []

    def fake_confusion(acc, label, ncls, ignore, hist):  # the confusion kernel's contract on the host
        pred = acc.argmax(1)
        lab = label.reshape(-1)
        keep = lab != ignore
        hist += torch.bincount(lab[keep] * ncls + pred[keep], minlength=ncls * ncls)
        seen.append(tuple(acc.shape))

    monkeypatch.setattr(Ev.K, "seg_confusion", fake_confusion)
    model = StubModel().train()
    m = Ev.fss_evaluate(model, [_stub_batch(2, 1, ["a.png", "b.png"]), _stub_batch(1, 0, ["c.png"])],
                        Cfg(num_classes=2, background=255), "cpu")
    assert not model.training and model.calls == [(2, 2, 3, 4, 6), (1, 2, 3, 4, 6)] and m.index == 2
    assert seen == [(2 * 4 * 6, 2), (1 * 4 * 6, 2)]
    # batch 1 predicts 1 everywhere (2 images: 12 bg rows... 6 bg pixels and 12 fg pixels each), batch 2 predicts 0
    assert m.hist.long().tolist() == [[6, 12], [12, 24]]
    bad = _stub_batch(1, 0, ["c.png"])
    del bad["s_depth"]
    with pytest.raises(KeyError, match="s_depth"):
        Ev.fss_evaluate(model, [bad], Cfg(num_classes=2, background=255), "cpu")
    bad = _stub_batch(1, 0, ["c.png"])
    bad["q_gt"] = bad["q_gt"][:, :3]
    with pytest.raises(ValueError, match="q_gt"):
        Ev.fss_evaluate(model, [bad], Cfg(num_classes=2, background=255), "cpu")


def test_meta_forward_argument_checks():
    """The rejections happen before the encoder runs (no GPU is touched)."""
    from dformer_amd.segmentor import EncoderDecoder
    base = dict(backbone="DFormerTrav-Base", decoder="ham", decoder_embed_dim=512, num_classes=2, drop_path_rate=0.0,
                bn_eps=1e-3, bn_momentum=0.1, background=255, aux_rate=0, alpha=0.5, temperature=1.0)
    ep = (torch.zeros(1, 2, 3, 32, 32), torch.zeros(1, 2, 1, 8), torch.zeros(1, 2, 32, 32), torch.zeros(1, 3, 32, 32),
          torch.zeros(1, 1, 8))
    model = EncoderDecoder(cfg=Cfg(base))
    assert model._fss_config() == (0.5, 1.0)
    with pytest.raises(ValueError, match="s_mask"):
        model.meta_forward(ep[0], ep[1], ep[2][:, :1], ep[3], ep[4])
    with pytest.raises(ValueError, match="q_gt"):
        model.meta_forward(*ep, torch.zeros(1, 16, 32))
    for name in ("alpha", "temperature"):
        model.cfg = Cfg({k: v for k, v in base.items() if k != name})
        with pytest.raises(ValueError, match=name):
            model.meta_forward(*ep)
    model.cfg = Cfg(base, temperature=0.0)
    with pytest.raises(ValueError, match="positive"):
        model.meta_forward(*ep)
    model.cfg = Cfg(base, num_classes=3)
    with pytest.raises(NotImplementedError, match="num_classes"):
        model.meta_forward(*ep)
    aux = EncoderDecoder(cfg=Cfg(base, aux_rate=0.4))
    with pytest.raises(NotImplementedError, match="aux"):
        aux.meta_forward(*ep)
    assert "255" in EncoderDecoder.meta_forward.__doc__ and "cfg.background" in EncoderDecoder.meta_forward.__doc__
