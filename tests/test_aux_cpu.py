"""The auxiliary FCN head (fcnhead.py:9-29, builder.py:138-143) on the host: which configs build it, its
state-dict keys / child order / optimizer groups against the reference's (tests/golden/e2e_tiny_aux*.npz,
oracle/golden_decoders.py / golden_e2e.py), checkpoint loading, and the argument validation of its two conv entry points."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import gen
from goldens import load


class Cfg(dict):
    __getattr__ = dict.__getitem__


def build(ncls=40, dec="ham", **extra):
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder=dec, decoder_embed_dim=512 if dec == "ham" else 64, num_classes=ncls,
              drop_path_rate=0.0, bn_eps=1e-3, bn_momentum=0.1, background=255, **extra)
    return EncoderDecoder(cfg=cfg, syncbn=False)


@pytest.mark.parametrize("name,ncls", [("e2e_tiny_aux", 40), ("e2e_tiny_aux37", 37)])
def test_aux_state_dict_children_and_groups_match_reference(name, ncls):
    from dformer_amd.train import group_weight
    g = load(name)
    model = build(ncls, aux_rate=0.4)
    sd = model.state_dict()
    # every key with its shape. (Inside decode_head the reference lists conv_seg first, this package last,
    # as before this head existed: keys are matched by name on load. The aux head's own keys, which come
    # last in both, are compared in order.)
    ref = {str(k): str(s) for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert {k: ",".join(str(d) for d in v.shape) for k, v in sd.items()} == ref
    assert [k for k in sd if k.startswith("aux_head.")] == [k for k in ref if k.startswith("aux_head.")]
    assert list(sd)[-9:] == [str(k) for k in g["sd_keys"][-9:]]
    assert [n for n, _ in model.named_children()] == ["encoder_backbone", "decode_head", "aux_head"]
    # builder.py:143 binds cfg.num_classes to the hidden width; the classifier stays 40 wide
    assert tuple(sd["aux_head.conv.0.weight"].shape) == (ncls, 128, 3, 3)
    assert tuple(sd["aux_head.classifier.weight"].shape) == (40, ncls, 1, 1)
    assert sd["aux_head.conv.1.num_batches_tracked"].dim() == 0
    bn = model.aux_head.conv[1]
    assert (bn.eps, bn.momentum) == (1e-3, 0.1)
    names = {id(p): n for n, p in model.named_parameters()}
    decay, nodecay = group_weight(model)
    assert [names[id(p)] for p in decay] == [str(k) for k in g["gw_decay"]]
    assert [names[id(p)] for p in nodecay] == [str(k) for k in g["gw_nodecay"]]


@pytest.mark.parametrize("extra", [dict(aux_rate=0), dict(aux_rate=0.0), dict()])
def test_no_aux_rate_builds_no_head(extra):
    import dformer_ref as R
    model = build(40, **extra)
    assert model.aux_head is None
    assert [n for n, _ in model.named_children()] == ["encoder_backbone", "decode_head"]
    sd = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert sd == R.segmentor_shapes("DFormer-Tiny", "ham", 40)


def test_mlp_decoder_ignores_aux_rate():
    model = build(37, dec="MLPDecoder", aux_rate=0.4)
    assert model.aux_head is None
    assert not any(k.startswith("aux_head.") for k in model.state_dict())


def test_syncbn_aux_head_uses_the_norm_layer_class():
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=40, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, aux_rate=0.4)
    m = EncoderDecoder(cfg=cfg, norm_layer=nn.SyncBatchNorm, syncbn=True)
    assert isinstance(m.aux_head.conv[1], nn.SyncBatchNorm) and m.aux_head.syncbn
    assert list(m.state_dict().keys()) == list(EncoderDecoder(cfg=cfg).state_dict().keys())


def test_load_model_with_aux_head_keys():
    from dformer_amd.checkpoint import load_model
    src = build(40, aux_rate=0.4)
    sd = src.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    state = {"model": {"module." + k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()}}
    dst = load_model(build(40, aux_rate=0.4), state)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, state["model"]["module." + k]), k
    with pytest.raises(RuntimeError):  # strict: a model without the head has nowhere to put aux_head.*
        load_model(build(40), state)


ENTRY = ["dfm_conv3s1_im2col", "dfm_conv3s1_col2im"]


@pytest.mark.parametrize("name", ENTRY)
def test_unknown_dtype_is_rejected_first(name):
    """The convention of tests/test_abi.py::test_unknown_dtype_is_rejected_first for the two new entry points."""
    from dformer_amd import _lib
    res, argtypes = _lib._SIGS[name]
    assert res is ctypes.c_int and argtypes[0] is ctypes.c_int
    args = [0 if t in (ctypes.c_int, ctypes.c_long) else None for t in argtypes]
    args[0] = 7
    st = getattr(_lib.lib, name)(*args)
    err = _lib.lib.dfm_last_error().decode()
    assert st == -2, (name, st, err)
    assert err.startswith(name + ": ") and "unsupported dtype 7" in err, err


def _args(name, **kw):
    """A valid call of `name` at B=1, 3x2, Cin=128 on fake (never dereferenced) pointers, with overrides."""
    a = dict(dtype=1, B=1, H=3, W=2, Cin=128, src=1 << 20, ld_src=None, dst=1 << 21, ld_dst=None)
    a.update(kw)
    cin = a["Cin"]
    wide, narrow = 9 * cin, cin
    if name == "dfm_conv3s1_im2col":
        ld_src = a["ld_src"] if a["ld_src"] is not None else narrow
        ld_dst = a["ld_dst"] if a["ld_dst"] is not None else wide
        return [a["dtype"], a["B"], a["H"], a["W"], cin, a["src"], ld_src, a["dst"], ld_dst, None]
    ld_src = a["ld_src"] if a["ld_src"] is not None else wide
    ld_dst = a["ld_dst"] if a["ld_dst"] is not None else narrow
    return [a["dtype"], a["B"], a["H"], a["W"], cin, a["src"], ld_src, a["dst"], ld_dst, 0, None]


@pytest.mark.parametrize("name", ENTRY)
@pytest.mark.parametrize("bad", [dict(Cin=20), dict(src=None), dict(dst=None), dict(B=0), dict(H=0), dict(W=-1),
                                 dict(Cin=0), dict(ld_src=8), dict(ld_dst=8), dict(src=(1 << 20) + 4)])
def test_bad_arguments_fail_before_any_launch(name, bad):
    from dformer_amd import _lib
    st = getattr(_lib.lib, name)(*_args(name, **bad))
    err = _lib.lib.dfm_last_error().decode()
    assert st == -1, (name, bad, st, err)
    assert err.startswith(name + ": "), err


def test_header_library_and_bindings_agree():
    import os
    import re
    from dformer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dformer_hip.h")).read()
    assert "fcnhead.py:19" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRY:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1])
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)
    assert _lib.lib.dfm_abi_version() == 13
