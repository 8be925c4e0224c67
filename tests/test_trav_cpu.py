"""The DFormerTrav backbone on the host (DFormer.py:308-457, builder.py:109-111): the algebra of the collapsed
laser-scan expansion against the reference's float64 goldens (oracle/golden_e2e.py), the state-dict keys,
child order and optimizer groups against the reference's, checkpoint loading, and the argument validation of
the two laser entry points."""
import ctypes

import numpy as np
import pytest
import torch

import trav_common as TC
from goldens import load, rel_err


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _expand_params(g):
    """The expansion's parameters of an expand golden as float64 leaves, under the module's own keys."""
    from dformer_amd.encoder import Attention1Dto2D
    B, N, L, Hout = [int(v) for v in g["meta"]]
    shapes = [(k, v.shape) for k, v in Attention1Dto2D(N, L, Hout, 64, 4).state_dict().items()]
    vals = TC.state_values(shapes, int(g["wmeta"][0]), float(g["wmeta"][1]))
    return {k: torch.from_numpy(np.asarray(v)).double().requires_grad_() for k, v in vals.items()}, (B, N, L, Hout)


@pytest.mark.parametrize("name", ["trav_expand_small", "trav_expand_full"])
def test_collapse_formula_matches_the_reference_module(name):
    """The fold + softmax-mean restatement (trav_common.fold64 / collapse64) in float64 against the
    reference's Attention1Dto2D: `s` (stored in float64) at 1e-9 rel-to-max, every parameter gradient through
    autograd of the restatement at 1e-6 (the goldens store gradients in float32: 6e-8 of rounding), and the
    hand-written gradient formulas (collapse_grads64) against that autograd."""
    import gen
    g = load(name)
    p, (B, N, L, Hout) = _expand_params(g)
    assert 1.0 <= float(g["cond"][0]) <= 20.0 and float(g["cond"][1]) >= 0.05
    x = torch.from_numpy(TC.scans(name, B, N))
    alpha, gh, c = TC.fold64(p)
    s, mean, var = TC.collapse64(x, alpha, gh, c)
    assert rel_err(s.detach(), g["s"]) < 1e-9
    gy = torch.from_numpy(gen.normal(name + "/gy", (B, 1, Hout, L)))[:, 0]
    (s[:, None, :].expand(B, Hout, L) * gy).sum().backward(retain_graph=True)
    seen = 0
    for k, v in g.items():
        if not k.startswith("grad/"):
            continue
        seen += 1
        got = p[k[5:]].grad if p[k[5:]].grad is not None else torch.zeros_like(p[k[5:]])
        if np.abs(v).max() == 0:
            assert torch.count_nonzero(got) == 0, k
        else:
            assert rel_err(got, v) < 1e-6, (k, rel_err(got, v))
    assert seen == 14
    ds, dalpha, dg, dc = TC.collapse_grads64(gy, gh.detach(), mean.detach(), var.detach())
    ga, gg, gc = torch.autograd.grad((s * ds).sum(), [alpha, gh, c])
    assert rel_err(dalpha, ga) < 1e-12 and rel_err(dg, gg) < 1e-12 and rel_err(dc, gc) < 1e-12


def build(expand=(24, 96, 64), **extra):
    from dformer_amd.encoder import Attention1Dto2D
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormerTrav-Base", decoder="ham", decoder_embed_dim=512, num_classes=2, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, **extra)
    model = EncoderDecoder(cfg=cfg, syncbn=False)
    if expand is not None:
        model.encoder_backbone.attn_expand_e = Attention1Dto2D(*expand, 64, 4)
    return model


NEVER_UPDATED = ["query1", "query2", "attn1.in_proj_weight", "attn1.in_proj_bias", "attn2.in_proj_weight",
                 "attn2.in_proj_bias"]
UPDATED = ["input_proj.weight", "input_proj.bias", "attn1.out_proj.weight", "attn1.out_proj.bias",
           "attn2.out_proj.weight", "attn2.out_proj.bias", "output_proj.weight", "output_proj.bias"]


def test_state_dict_children_and_groups_match_reference():
    from dformer_amd.train import group_weight
    g = load("e2e_trav_small")
    model = build()
    sd = model.state_dict()
    ref = {str(k): str(s) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert {k: ",".join(str(d) for d in v.shape) for k, v in sd.items()} == ref
    # the backbone's keys in the reference's order (inside decode_head the reference lists conv_seg first,
    # this package last: tests/test_aux_cpu.py)
    enc = [k for k in sd if k.startswith("encoder_backbone.")]
    assert enc == [k for k in ref if k.startswith("encoder_backbone.")]
    assert not [k for k in sd if "stem_e_fc" in k]
    bb = model.encoder_backbone
    assert [n for n, _ in bb.named_children()] == ["downsample_layers", "attn_expand_e", "downsample_layers_e",
                                                   "stages"]
    pre = "encoder_backbone.attn_expand_e."
    assert [k[len(pre):] for k in sd if k.startswith(pre)] == [
        "query1", "query2", "input_proj.weight", "input_proj.bias", "attn1.in_proj_weight", "attn1.in_proj_bias",
        "attn1.out_proj.weight", "attn1.out_proj.bias", "attn2.in_proj_weight", "attn2.in_proj_bias",
        "attn2.out_proj.weight", "attn2.out_proj.bias", "output_proj.weight", "output_proj.bias"]
    assert isinstance(bb.attn_expand_e.attn1.out_proj, torch.nn.Linear)
    assert isinstance(bb.attn_expand_e.attn2.out_proj, torch.nn.Linear)
    assert not [m for m in model.modules() if isinstance(m, torch.nn.MultiheadAttention)]
    names = {id(p): n for n, p in model.named_parameters()}
    decay, nodecay = group_weight(model)
    assert [names[id(p)] for p in decay] == [str(k) for k in g["gw_decay"]]
    assert [names[id(p)] for p in nodecay] == [str(k) for k in g["gw_nodecay"]]
    grouped = {names[id(p)] for p in decay + nodecay}
    assert not [n for n in NEVER_UPDATED if pre + n in grouped]  # the reference's group_weight quirk
    assert all(pre + n in grouped for n in UPDATED)


def test_default_expansion_is_the_references():
    from dformer_amd.encoder import DFormerTrav
    bb = build(expand=None).encoder_backbone
    assert isinstance(bb, DFormerTrav) and bb.expand == (360, 640, 480)
    e = bb.attn_expand_e
    assert (e.input_len, e.mid_len, e.output_len, e.embed_dim, e.num_heads) == (360, 640, 480, 64, 4)
    assert tuple(e.query1.shape) == (640, 64) and tuple(e.query2.shape) == (480, 64)
    small = DFormerTrav(expand=(12, 10, 6)).attn_expand_e
    assert (small.input_len, small.mid_len, small.output_len) == (12, 10, 6)


def test_unknown_backbone_still_fails():
    from dformer_amd.segmentor import BACKBONES
    assert "DFormerTrav-Base" in BACKBONES and BACKBONES["DFormerTrav-Base"][1] == [64, 128, 256, 512]


def test_reference_layout_checkpoint_round_trips():
    from dformer_amd.checkpoint import load_model, load_pretrained_backbone
    g = load("e2e_trav_small")
    src = build()
    TC.load_values(src, int(g["wmeta"][0]), float(g["wmeta"][1]))
    state = {"model": {"module." + k: v.clone() for k, v in src.state_dict().items()}}
    dst = load_model(build(), state)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, state["model"]["module." + k]), k
    # DFormerTrav.init_weights (DFormer.py:408-427): the weights under `model`, `backbone.` stripped,
    # non-strict, nothing frozen
    pre = "encoder_backbone."
    ck = {"model": {"backbone." + k[len(pre):]: v.clone() for k, v in src.state_dict().items() if k.startswith(pre)}}
    ck["model"]["backbone.not_a_key"] = torch.zeros(1)
    fresh = build().encoder_backbone
    missing, unexpected = load_pretrained_backbone(fresh, ck)
    assert missing == [] and unexpected == ["not_a_key"]
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, src.state_dict()[pre + k]), k
    assert all(p.requires_grad for p in fresh.parameters())


def test_scan_models_reject_resizing_paths():
    """A scan cannot be resized, cropped or flipped: sliding windows, scales != 1 and flips raise before any
    kernel runs (the reference asserts / crashes there, val_mm.py:293, 362-372)."""
    from dformer_amd import evaluate as E
    model = build()
    rgb, scan = torch.zeros(1, 3, 64, 96), torch.zeros(1, 1, 24)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.msf_scores(model, rgb, scan, 2, [0.5, 1.0], False)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.msf_scores(model, rgb, scan, 2, [1.0], True)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.msf_scores(model, rgb, scan, 2, [1.0], False, crop_size=(32, 32), stride_rate=0.5)
    cfg = Cfg(num_classes=2, background=255, eval_crop_size=(32, 32), eval_stride_rate=0.5)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.slide_inference(model, rgb, scan, cfg)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.evaluate(model, [], cfg, "cpu", sliding=True)


# ------------------------------------------------------------------------------------- the C ABI
def _fwd_args(**kw):
    a = dict(B=2, N=12, L=10, Hh=4, Hout=6, x=1 << 20, alpha=1 << 21, g=1 << 22, c=1 << 23, s=1 << 24, mean=1 << 25,
             var=1 << 26, plane=1 << 27, stream=None)
    a.update(kw)
    return list(a.values())


def _bwd_args(**kw):
    a = dict(B=2, L=10, Hh=4, Hout=6, dplane=1 << 20, g=1 << 21, mean=1 << 22, var=1 << 23, ds=1 << 24,
             dalpha=1 << 25, dg=1 << 26, dc=1 << 27, workspace=1 << 28, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad,says", [
    (dict(N=8193), "N=8193 exceeds the 8192"), (dict(N=0), "bad argument"), (dict(B=0), "bad argument"),
    (dict(L=0), "bad argument"), (dict(Hout=0), "bad argument"), (dict(Hh=0), "Hh=0"), (dict(Hh=9), "Hh=9"),
    (dict(x=None), "null pointer"), (dict(alpha=None), "null pointer"), (dict(g=None), "null pointer"),
    (dict(c=None), "null pointer"), (dict(s=None), "null pointer"), (dict(plane=None), "null pointer"),
    (dict(mean=None), "mean and var go together"), (dict(var=None), "mean and var go together")])
def test_fwd_bad_arguments_fail_before_any_launch(bad, says):
    from dformer_amd import _lib
    st = _lib.lib.dfm_laser_expand_fwd(*_fwd_args(**bad))
    err = _lib.lib.dfm_last_error().decode()
    assert st == -1, (bad, st, err)
    assert err.startswith("dfm_laser_expand_fwd: ") and says in err, err


@pytest.mark.parametrize("bad,says", [
    (dict(B=0), "bad argument"), (dict(L=-1), "bad argument"), (dict(Hout=0), "bad argument"), (dict(Hh=9), "Hh=9"),
    (dict(dplane=None), "null pointer"), (dict(g=None), "null pointer"), (dict(mean=None), "null pointer"),
    (dict(var=None), "null pointer"), (dict(ds=None), "null pointer"), (dict(dalpha=None), "null pointer"),
    (dict(dg=None), "null pointer"), (dict(dc=None), "null pointer"), (dict(workspace=None), "null pointer")])
def test_bwd_bad_arguments_fail_before_any_launch(bad, says):
    from dformer_amd import _lib
    st = _lib.lib.dfm_laser_expand_bwd(*_bwd_args(**bad))
    err = _lib.lib.dfm_last_error().decode()
    assert st == -1, (bad, st, err)
    assert err.startswith("dfm_laser_expand_bwd: ") and says in err, err


def test_header_library_and_bindings_agree():
    import os
    import re
    from dformer_amd import _lib
    from dformer_amd import kernels as K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dformer_hip.h")).read()
    assert "DFormer.py:308-339" in src
    assert int(re.search(r"#define\s+DFM_LASER_MAX_N\s+(\d+)", src).group(1)) == K.LASER_MAX_N == 8192
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("dfm_laser_expand_fwd", "dfm_laser_expand_bwd"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1])
        assert _lib._SIGS[name][0] is ctypes.c_int
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert re.search(r"\bsize_t\s+dfm_laser_expand_bwd_workspace\s*\(\s*int\s+L\s*,\s*int\s+Hh\s*\)\s*;", src)
    ws = _lib.lib.dfm_laser_expand_bwd_workspace
    assert ws(640, 4) == 10 * 9 * 4 and ws(1, 1) == 36 and ws(0, 4) == 0 and ws(10, 9) == 0
    assert _lib.lib.dfm_abi_version() == 13 == _lib.ABI_VERSION  # new symbols, no layout change


def test_constructor_rejects_what_the_kernel_cannot_run():
    from dformer_amd.encoder import Attention1Dto2D
    with pytest.raises(ValueError, match="8192"):
        Attention1Dto2D(input_len=8193)
    with pytest.raises(ValueError, match="heads"):
        Attention1Dto2D(embed_dim=64, num_heads=16)
