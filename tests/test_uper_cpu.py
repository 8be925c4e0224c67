"""The UPerNet decoder (UPernet.py:8-146, builder.py:145-152) on the host: the new entry points resolve and
validate their arguments before touching a device, `decoder="UPernet"` builds, and its state-dict keys / shapes
and optimizer groups equal the reference's in order (tests/golden/e2e_tiny_uper.npz, oracle/golden_decoders.py / golden_e2e.py)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from goldens import load

NEW = ["dfm_conv3s1_igemm_supported", "dfm_conv3s1_igemm_fwd", "dfm_conv3_weight_pack_dgrad",
       "dfm_conv3s1_igemm_wgrad_workspace_size", "dfm_conv3s1_igemm_wgrad", "dfm_ppm_pool_fwd", "dfm_ppm_pool_bwd"]
X, WP, Y, WS = 1 << 20, 1 << 21, 1 << 22, 1 << 23  # fake, 16-byte aligned, never dereferenced


class Cfg(dict):
    __getattr__ = dict.__getitem__


def build(dec="UPernet", **extra):
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder=dec, decoder_embed_dim=512, num_classes=40, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, **extra)
    return EncoderDecoder(cfg=cfg, syncbn=False)


def test_new_symbols_resolve_and_abi_stays_13():
    from dformer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dformer_hip.h")).read()
    assert "UPernet.py:30,44,52" in src and "UPernet.py:126-133" in src  # each cites the line it replaces
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert _lib.lib.dfm_abi_version() == 13 == _lib.ABI_VERSION


def test_supported_query():
    from dformer_amd import _lib
    q = _lib.lib.dfm_conv3s1_igemm_supported
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        assert q(dt, 512, 512) == 1 and q(dt, 2304, 512) == 1 and q(dt, 2624, 512) == 1 and q(dt, 8, 8) == 1
        assert q(dt, 12, 64) == 0 and q(dt, 64, 12) == 0 and q(dt, 0, 8) == 0
    assert q(7, 64, 64) == 0


def _fwd(**kw):
    a = dict(dtype=1, B=1, H=3, W=2, Cin=64, Cout=32, x=X, ldx=None, wp=WP, bias=None, y=Y, ldy=None)
    a.update(kw)
    ldx = a["ldx"] if a["ldx"] is not None else a["Cin"]
    ldy = a["ldy"] if a["ldy"] is not None else a["Cout"]
    return [a["dtype"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["x"], ldx, a["wp"], a["bias"], a["y"], ldy, 0,
            None]


@pytest.mark.parametrize("bad", [dict(x=None), dict(wp=None), dict(y=None), dict(ldx=56), dict(ldy=24), dict(ldx=68),
                                 dict(Cin=12), dict(Cout=20), dict(B=0), dict(H=0), dict(W=-1), dict(x=X + 4)])
def test_conv_fwd_bad_arguments_fail_before_any_launch(bad):
    from dformer_amd import _lib
    st = _lib.lib.dfm_conv3s1_igemm_fwd(*_fwd(**bad))
    err = _lib.lib.dfm_last_error().decode()
    assert st == -1, (bad, st, err)
    assert err.startswith("dfm_conv3s1_igemm_fwd: "), err


def _wgrad(**kw):
    a = dict(dtype=1, B=3, H=17, W=23, Cin=32, Cout=16, dy=Y, lddy=None, x=X, ldx=None, dwp=WP, db=None, ws=WS,
             ws_bytes=None)
    a.update(kw)
    return a


def test_conv_wgrad_bad_arguments_and_workspace():
    from dformer_amd import _lib
    lib = _lib.lib

    def call(**kw):
        a = _wgrad(**kw)
        need = lib.dfm_conv3s1_igemm_wgrad_workspace_size(a["dtype"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"],
                                                          int(a["db"] is not None))
        wsb = a["ws_bytes"] if a["ws_bytes"] is not None else need
        ldx = a["ldx"] if a["ldx"] is not None else a["Cin"]
        lddy = a["lddy"] if a["lddy"] is not None else a["Cout"]
        st = lib.dfm_conv3s1_igemm_wgrad(a["dtype"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["dy"], lddy,
                                         a["x"], ldx, a["dwp"], a["db"], a["ws"], wsb, None)
        return st, lib.dfm_last_error().decode(), need

    _, _, need = call(dy=None)
    assert need > 0  # 3 x 17 x 23 pixels over three column tiles: split over pixels, across the images
    assert need % 4 == 0 and need >= 2 * 16 * 9 * 32 * 4
    for bad in (dict(dy=None), dict(x=None), dict(dwp=None), dict(ldx=24), dict(lddy=8), dict(Cin=12),
                dict(ws_bytes=need - 4), dict(ws=None), dict(B=0)):
        st, err, _ = call(**bad)
        assert st == -1, (bad, st, err)
        assert err.startswith("dfm_conv3s1_igemm_wgrad: "), err
    assert lib.dfm_conv3s1_igemm_wgrad_workspace_size(1, 1, 2, 3, 64, 64, 1) == 0  # 6 pixels: unsplit
    assert lib.dfm_conv3s1_igemm_wgrad_workspace_size(1, 1, 2, 3, 12, 64, 1) == 0  # unsupported: nothing to size


@pytest.mark.parametrize("name", ["dfm_ppm_pool_fwd", "dfm_ppm_pool_bwd"])
@pytest.mark.parametrize("bad", [dict(C=12), dict(src=None), dict(dst=None), dict(s=(0, 2, 3, 6)), dict(s=(1, 2, 3, 17)),
                                 dict(s=(1, 0, 3, 0)), dict(ld=32), dict(B=0)])
def test_pool_bad_arguments_fail_before_any_launch(name, bad):
    from dformer_amd import _lib
    a = dict(B=2, H=5, W=7, C=40, s=(1, 2, 3, 6), src=X, dst=Y, ld=40)
    a.update(bad)
    args = [1, a["B"], a["H"], a["W"], a["C"], *a["s"], a["src"], a["ld"], a["dst"], a["ld"]]
    args += [None] if name.endswith("fwd") else [0, None]
    st = getattr(_lib.lib, name)(*args)
    err = _lib.lib.dfm_last_error().decode()
    assert st == -1, (name, bad, st, err)
    assert err.startswith(name + ": "), err


@pytest.mark.parametrize("name,pos", [("dfm_conv3s1_igemm_fwd", 0), ("dfm_conv3_weight_pack_dgrad", 0),
                                      ("dfm_conv3s1_igemm_wgrad", 0), ("dfm_ppm_pool_fwd", 0), ("dfm_ppm_pool_bwd", 0)])
def test_unknown_dtype_is_rejected_first(name, pos):
    from dformer_amd import _lib
    res, argtypes = _lib._SIGS[name]
    args = [0 if t in (ctypes.c_int, ctypes.c_long, ctypes.c_size_t) else None for t in argtypes]
    args[pos] = 7
    st = getattr(_lib.lib, name)(*args)
    err = _lib.lib.dfm_last_error().decode()
    assert st == -2 and err.startswith(name + ": ") and "unsupported dtype 7" in err, (st, err)


def test_upernet_builds_with_reference_keys_shapes_and_groups():
    from dformer_amd.decoders import FCNHead, PPM, UPerHead
    from dformer_amd.train import group_weight
    g = load("e2e_tiny_uper")
    model = build()
    assert isinstance(model.decode_head, UPerHead) and isinstance(model.decode_head.psp_modules, PPM)
    assert isinstance(model.aux_head, FCNHead) and model.aux_index == 2
    assert [n for n, _ in model.named_children()] == ["encoder_backbone", "decode_head", "aux_head"]
    assert [n for n, _ in model.decode_head.named_children()] == ["psp_modules", "bottleneck", "lateral_convs",
                                                                  "fpn_convs", "fpn_bottleneck", "conv_seg"]
    assert not hasattr(model.decode_head, "reference_children")
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["sd_keys"]]  # the reference's keys, in the reference's order
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in g["sd_shapes"]]
    assert tuple(sd["decode_head.bottleneck.0.weight"].shape) == (512, 256 + 4 * 512, 3, 3)
    assert tuple(sd["decode_head.psp_modules.3.1.bias"].shape) == (512,)  # every conv has a bias ahead of its BN
    for m in list(model.decode_head.modules()) + list(model.aux_head.modules()):
        if isinstance(m, nn.BatchNorm2d):
            assert (m.eps, m.momentum) == (1e-3, 0.1)
    names = {id(p): n for n, p in model.named_parameters()}
    decay, nodecay = group_weight(model)
    assert [names[id(p)] for p in decay] == [str(k) for k in g["gw_decay"]]
    assert [names[id(p)] for p in nodecay] == [str(k) for k in g["gw_nodecay"]]


@pytest.mark.parametrize("extra", [dict(aux_rate=0), dict(aux_rate=0.1), dict()])
def test_upernet_aux_rate_is_hard_coded(extra):
    model = build(**extra)
    assert model.aux_rate == 0.4 and model.aux_head is not None


def test_upernet_refuses_meta_forward_and_other_decoders_still_raise():
    model = build()
    model.cfg["num_classes"] = 2
    with pytest.raises(NotImplementedError, match="aux head"):
        model._fss_config()
    for dec in ("deeplabv3+", "nl", "fcn"):
        with pytest.raises(NotImplementedError, match="outside the hot path"):
            build(dec)


def test_uperhead_constructor_follows_the_reference():
    from dformer_amd.decoders import UPerHead
    head = UPerHead([16, 32, 64, 96], num_classes=40, channels=32, pool_scales=(1, 2, 3, 6),
                    norm_layer=nn.BatchNorm2d, dropout_ratio=0.1, align_corners=False)
    keys = list(head.state_dict())
    assert keys[:2] == ["psp_modules.0.1.weight", "psp_modules.0.1.bias"] and keys[-2:] == ["conv_seg.weight",
                                                                                             "conv_seg.bias"]
    assert "psp_modules.3.2.running_var" in keys and "lateral_convs.2.1.weight" in keys
    assert "fpn_convs.0.0.bias" in keys and "fpn_bottleneck.1.num_batches_tracked" in keys
    assert not any("dropout" in k for k in keys)
    with pytest.raises(NotImplementedError):
        UPerHead([16, 32, 64, 96], channels=32, align_corners=True)
    with pytest.raises(NotImplementedError):
        UPerHead([16, 32, 64, 100], channels=32)  # 100 + 4*32 is no multiple of 8
    assert torch.is_tensor(head.conv_seg.bias)
