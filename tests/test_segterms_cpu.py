"""The criterion library without a GPU: libdformer_criterion.so exports what include/dformer_criterion.h
declares and what dformer_amd/criterion.py binds, holds exactly the kernels listed here, is loaded only on first
use of a focal or region option, rejects bad arguments before any launch; and losses.FusedSegLoss.forward (the
definition of focal_gamma / region) against an independent float64 restatement written as explicit loops."""
import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dformer_criterion.h")
IGNORE = 255

# Every kernel instantiation of libdformer_criterion.so, with the cases of tests/test_segterms_gpu.py that run
# it (every case of test_terms_against_float64 runs the forward, reduce, final and backward kernels of its dtype).
KERNELS = [
    "seg_terms_bwd_kernel<f16_t>",           # test_terms_against_float64[float16-*], test_saturated_logits
    "seg_terms_bwd_kernel<float>",           # test_terms_against_float64[float32-*], test_encoder_decoder_end_to_end
    "seg_terms_bwd_kernel<unsigned short>",  # test_terms_against_float64[bfloat16-*]
    "seg_terms_final_kernel",                # every forward
    "seg_terms_fwd_kernel<f16_t>",           # test_terms_against_float64[float16-*], test_saturated_logits
    "seg_terms_fwd_kernel<float>",           # test_terms_against_float64[float32-*], test_stats
    "seg_terms_fwd_kernel<unsigned short>",  # test_terms_against_float64[bfloat16-*]
    "seg_terms_reduce_kernel",               # every forward
]


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dfc_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return decls


# ---------------------------------------------------------------- header, bindings, library contents
def test_binding_signatures_match_header():
    from dformer_amd import criterion
    d = declared()
    assert d == {"dfc_last_error": 0, "dfc_abi_version": 0, "dfc_seg_terms_workspace": 6, "dfc_seg_terms_fwd": 16,
                 "dfc_seg_terms_bwd": 18}
    assert set(d) == set(criterion._SIGS), set(d) ^ set(criterion._SIGS)
    for name, n in d.items():
        assert len(criterion._SIGS[name][1]) == n, (name, n, len(criterion._SIGS[name][1]))
    raw = ctypes.CDLL(criterion.LIB_PATH)
    for name in d:
        assert hasattr(raw, name), name
    exported = sorted(s for s in kv._symtab_names(criterion.LIB_PATH) if s.startswith("dfc_"))
    assert exported == sorted(d), exported
    assert criterion.lib.dfc_abi_version() == 1 == criterion.ABI_VERSION
    src = open(HEADER).read()
    from dformer_amd import losses
    assert f"#define DFC_MAX_CLASSES {criterion.MAX_CLASSES}\n" in src and criterion.MAX_CLASSES == losses.MAX_CLASSES
    assert f"#define DFC_MAX_DIM {criterion.MAX_DIM} " in src and f"#define DFC_MAX_BATCH {criterion.MAX_BATCH}\n" in src
    # the dtype codes are the model library's (criterion.py passes _lib.dtype_code)
    from dformer_amd import _lib
    for name, code in (("DFC_F32", _lib.F32), ("DFC_BF16", _lib.BF16), ("DFC_F16", _lib.F16)):
        assert f"#define {name} {code}\n" in src


def test_library_kernels_and_symbols():
    from dformer_amd import criterion
    names, raw = kv.library_variants(criterion.LIB_PATH)
    assert raw == len(names) and names == sorted(KERNELS), names
    symbols = kv._symtab_names(criterion.LIB_PATH)
    assert not [s for s in symbols if s.startswith(("dfm_", "dfd_"))], "the criterion library defines no dfm_* / dfd_*"
    raw_lib = ctypes.CDLL(criterion.LIB_PATH)
    assert not hasattr(raw_lib, "dfm_abi_version") and not hasattr(raw_lib, "dfd_abi_version")


def test_desc_layout_matches_c_struct(tmp_path):
    import shutil
    from dformer_amd import criterion
    assert ctypes.sizeof(criterion.TermsDesc) == 6 * 4
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    names = [f[0] for f in criterion.TermsDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(DfcTermsDesc));' % HEADER
    for n in names:
        src += 'printf(" %%zu", offsetof(DfcTermsDesc, %s));' % n
    src += "return 0;}\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(criterion.TermsDesc)
    assert vals[1:] == [getattr(criterion.TermsDesc, n).offset for n in names]


def test_loader_refuses_another_abi():
    from dformer_amd import criterion

    class Stub:
        @staticmethod
        def dfc_abi_version():
            return 2

    with pytest.raises(ImportError) as e:
        criterion.check_abi(Stub)
    assert "2" in str(e.value) and criterion.LIB_PATH in str(e.value)
    criterion.check_abi(criterion.lib)


def test_default_criterion_does_not_map_the_library():
    """import dformer_amd.segmentor + a default FusedSegLoss and its CPU forward map the model library alone; a
    criterion with a region term still maps nothing until its fused path runs; importing the module maps it."""
    code = ("import torch, dformer_amd.segmentor\n"
            "from dformer_amd.losses import FusedSegLoss\n"
            "pred, tgt = torch.randn(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)\n"
            "FusedSegLoss()(pred, tgt)\n"
            "m = open('/proc/self/maps').read()\n"
            "print(int('libdformer_hip.so' in m), int('libdformer_criterion.so' in m))\n"
            "FusedSegLoss(focal_gamma=2.0, region='dice')(pred, tgt)\n"
            "print(int('libdformer_criterion.so' in open('/proc/self/maps').read()))\n"
            "import dformer_amd.criterion\n"
            "print(int('libdformer_criterion.so' in open('/proc/self/maps').read()))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["1", "0", "0", "1"], out


# ---------------------------------------------------------------- validation before any launch
GOOD = dict(dtype=0, B=2, h=5, w=7, ncls=40, H=40, W=56, ignore=255, gamma=2.0, alpha=0.3, beta=0.7, smooth=1.0,
            has_pixel=1, has_region=1, region_weight=1.0)
BAD = [dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(w=-3), dict(H=0), dict(W=-1), dict(H=16385),
       dict(h=41), dict(w=57), dict(ncls=0), dict(ncls=65), dict(ncls=-2), dict(dtype=3), dict(dtype=-1),
       dict(gamma=-0.5), dict(gamma=math.inf), dict(gamma=math.nan), dict(smooth=0.0), dict(smooth=-1.0),
       dict(alpha=-0.1), dict(beta=-0.1), dict(alpha=0.0, beta=0.0), "null_logits", "null_label", "null_out",
       "null_stats", "null_desc"]


def call(entry, bad):
    """The entry point with fake pointers that are never dereferenced -> (status, message)."""
    from dformer_amd import criterion as C
    v = dict(GOOD)
    if isinstance(bad, dict):
        v.update(bad)
    fake = ctypes.c_void_p(1 << 20)
    ptrs = dict(logits=fake, label=fake, out=fake, stats=fake, ws=fake, dl=fake)
    desc = C.TermsDesc(v["gamma"], v["alpha"], v["beta"], v["smooth"], v["has_pixel"], v["has_region"])
    if isinstance(bad, str):
        if bad == "null_desc":
            desc = None
        else:
            ptrs[bad[5:]] = None
    head = [v["dtype"], v["B"], v["h"], v["w"], v["ncls"], ptrs["logits"], v["H"], v["W"], ptrs["label"], v["ignore"],
            None, desc]
    if entry == "dfc_seg_terms_fwd":
        st = C.lib.dfc_seg_terms_fwd(*head, ptrs["ws"], ptrs["stats"], ptrs["out"], None)
    else:
        st = C.lib.dfc_seg_terms_bwd(*head, ptrs["stats"], ptrs["out"], None, v["region_weight"], ptrs["dl"], None)
    return st, C.lib.dfc_last_error()


@pytest.mark.parametrize("entry", ["dfc_seg_terms_fwd", "dfc_seg_terms_bwd"])
@pytest.mark.parametrize("bad", BAD, ids=lambda b: b if isinstance(b, str) else "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_argument_is_rejected(entry, bad):
    from dformer_amd import criterion as C
    st, msg = call(entry, bad)
    assert st == -1
    assert msg.startswith(entry.encode() + b": "), msg
    with pytest.raises(RuntimeError):
        C.check(st, entry)


def test_bad_arguments_of_one_entry_point_only():
    from dformer_amd import criterion as C
    for rw in (-1.0, math.inf, math.nan):
        st, msg = call("dfc_seg_terms_bwd", dict(region_weight=rw))
        assert st == -1 and msg.startswith(b"dfc_seg_terms_bwd: ")
    st, msg = call("dfc_seg_terms_bwd", "null_dl")
    assert st == -1 and msg.startswith(b"dfc_seg_terms_bwd: ")
    st, msg = call("dfc_seg_terms_fwd", "null_ws")
    assert st == -1 and msg.startswith(b"dfc_seg_terms_fwd: ")
    # the region parameters are not looked at without a region term
    assert C.lib.dfc_seg_terms_workspace(2, 5, 7, 40, 40, 56) > 0
    for bad in (dict(B=0), dict(ncls=65), dict(H=16385), dict(h=0)):
        v = dict(GOOD, **bad)
        assert C.lib.dfc_seg_terms_workspace(v["B"], v["h"], v["w"], v["ncls"], v["H"], v["W"]) == 0


def test_workspace_is_a_small_fraction_of_the_full_resolution_logits():
    from dformer_amd import criterion as C
    for B, ncls in ((16, 40), (16, 2), (2, 64)):
        ws = C.lib.dfc_seg_terms_workspace(B, 60, 80, ncls, 480, 640)
        assert ws <= B * ncls * 480 * 640 * 4 // 32, (B, ncls, ws)


# ---------------------------------------------------------------- constructor
def test_constructor_rejects():
    from dformer_amd.losses import FusedSegLoss
    bad = [dict(focal_gamma=-1.0), dict(focal_gamma=math.inf), dict(focal_gamma=math.nan),
           dict(focal_gamma=2.0, label_smoothing=0.1), dict(focal_gamma=2.0, ohem_thresh=0.7, ohem_min_kept=10),
           dict(region="jaccard"), dict(region=True), dict(region="tversky", region_smooth=0.0),
           dict(region="tversky", region_smooth=-1.0), dict(region="tversky", region_alpha=-0.1),
           dict(region="tversky", region_beta=-0.1), dict(region="tversky", region_alpha=0.0, region_beta=0.0),
           dict(region="tversky", region_weight=-1.0), dict(region="tversky", region_weight=math.inf),
           dict(region="dice", region_alpha=0.5), dict(region="dice", region_beta=0.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            FusedSegLoss(**kw)
    ok = FusedSegLoss(focal_gamma=2.0, region="tversky", region_weight=0.0)
    assert ok.has_terms() and ok.region_options() == (0.3, 0.7, 1.0)
    assert len(ok.kernel_options(torch.device("cpu"))) == 4
    r = repr(ok)
    assert "focal_gamma=2.0" in r and "region='tversky'" in r and "region_alpha=0.3" in r
    assert not FusedSegLoss().has_terms() and "focal" not in repr(FusedSegLoss())
    # label smoothing and mining go with a region term (the pixel term stays SegLossFn's)
    FusedSegLoss(region="dice", label_smoothing=0.1, ohem_thresh=0.7, ohem_min_kept=10)


def make_case(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    pred = 3 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    tgt = torch.randint(0, C, (B, H, W), generator=g)
    tgt[-1][tgt[-1] == C - 1] = 0  # a class absent from one image
    tgt[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    weight = 0.5 + 1.5 * torch.rand(C, generator=g)
    weight[C // 2] = 0.0
    return pred, tgt, weight


def test_dice_is_tversky_with_halves():
    from dformer_amd.losses import FusedSegLoss
    pred, tgt, weight = make_case(3, 5, 12, 16, 1)
    a = FusedSegLoss(weight=weight, region="dice")(pred, tgt)
    b = FusedSegLoss(weight=weight, region="tversky", region_alpha=0.5, region_beta=0.5)(pred, tgt)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- the definition, restated
def restated(pred, tgt, weight, gamma, region, rw, smooth):
    """tversky_loss.py:25-57 in shape: explicit loops over images and classes, float64; the focal term per
    pixel from log-softmax; with gamma = 0 the plain weighted cross-entropy."""
    B, C, H, W = pred.shape
    logp = pred - torch.logsumexp(pred, dim=1, keepdim=True)
    prob = logp.exp()
    total, count = pred.new_zeros(()), 0
    for b in range(B):
        for c in range(C):
            mine = tgt[b] == c
            lq = logp[b, c][mine]
            q = lq.exp()
            total = total + (weight[c].double() * (1.0 - q) ** gamma * -lq).sum()
            count += int(mine.sum())
    loss = total / max(count, 1)
    if region is not None:
        alpha, beta = region
        acc = pred.new_zeros(())
        for b in range(B):
            valid = (tgt[b] != IGNORE).double()
            per_image = pred.new_zeros(())
            for c in range(C):
                p = prob[b, c]
                t = (tgt[b] == c).double()
                tp = (p * t * valid).sum()
                fp = (p * (1 - t) * valid).sum()
                fn = ((1 - p) * t * valid).sum()
                per_image = per_image + weight[c].double() * (1 - (tp + smooth) / (tp + alpha * fp + beta * fn + smooth))
            acc = acc + per_image / C
        loss = loss + rw * acc / B
    return loss


@pytest.mark.parametrize("opts", [dict(focal_gamma=2.0), dict(focal_gamma=0.5), dict(region="tversky"),
                                  dict(region="dice", region_smooth=0.5),
                                  dict(focal_gamma=2.0, region="tversky", region_weight=0.7, region_alpha=0.4,
                                       region_beta=0.6)],
                         ids=["focal2", "focal0.5", "tversky", "dice", "both"])
@pytest.mark.parametrize("shape", [(3, 5, 12, 16), (2, 2, 10, 14)])
def test_forward_is_the_restated_definition(shape, opts):
    from dformer_amd.losses import FusedSegLoss
    pred, tgt, weight = make_case(*shape, seed=7)
    assert (tgt == IGNORE).any() and not (tgt[-1] == shape[1] - 1).any() and (weight == 0).sum() == 1
    crit = FusedSegLoss(weight=weight, **opts)
    x = pred.clone().requires_grad_()
    loss = crit(x, tgt)
    loss.backward()
    y = pred.clone().requires_grad_()
    region = None if crit.region is None else (crit.region_alpha, crit.region_beta)
    ref = restated(y, tgt, weight, crit.focal_gamma, region, crit.region_weight, crit.region_smooth)
    ref.backward()
    assert loss.dtype == torch.float64
    assert abs(loss.item() - ref.item()) <= 1e-10 * abs(ref.item()), (loss.item(), ref.item())
    gerr = ((x.grad - y.grad).abs().max() / y.grad.abs().max()).item()
    assert gerr <= 1e-10, gerr
    # without weights the definition is the weighted one at w = 1
    ones = torch.ones(shape[1])
    a = FusedSegLoss(**opts)(pred, tgt)
    b = restated(pred, tgt, ones, crit.focal_gamma, region, crit.region_weight, crit.region_smooth)
    assert abs(a.item() - b.item()) <= 1e-10 * abs(b.item())


# ---------------------------------------------------------------- special cases
def test_neutral_options_are_the_existing_forward():
    from dformer_amd.losses import FusedSegLoss
    pred, tgt, weight = make_case(3, 5, 12, 16, 3)
    pred = pred.float()
    for kw in (dict(), dict(weight=weight, label_smoothing=0.1), dict(weight=weight, ohem_thresh=0.7, ohem_min_kept=50)):
        a = FusedSegLoss(**kw)(pred, tgt)
        b = FusedSegLoss(focal_gamma=0.0, region=None, **kw)(pred, tgt)
        kept = FusedSegLoss(**kw).mined_target(pred, tgt)
        per = F.cross_entropy(pred, kept, weight=kw.get("weight"), reduction="none", ignore_index=IGNORE,
                              label_smoothing=kw.get("label_smoothing", 0.0))
        want = per.sum() / (kept != IGNORE).sum().clamp_min(1)
        assert torch.equal(a, b) and torch.equal(a, want)


@pytest.mark.parametrize("opts", [dict(focal_gamma=2.0), dict(region="tversky"), dict(focal_gamma=0.5, region="dice")])
def test_all_ignored_is_zero(opts):
    """No valid pixel: T_bc = s / s = 1 for every class, the pixel term is 0 / max(0, 1)."""
    from dformer_amd.losses import FusedSegLoss
    pred = torch.randn(2, 4, 6, 8, requires_grad=True)
    tgt = torch.full((2, 6, 8), IGNORE)
    loss = FusedSegLoss(**opts)(pred, tgt)
    loss.backward()
    assert loss.item() == 0.0 and torch.all(pred.grad == 0)


def test_meta_forward_and_check_criterion_keep_their_contract():
    """The segmentor accepts the new options like any FusedSegLoss (ignore_index and weight width are checked)."""
    from dformer_amd.losses import FusedSegLoss
    from dformer_amd.segmentor import _check_criterion
    _check_criterion(FusedSegLoss(focal_gamma=2.0, region="dice"), 255)
    with pytest.raises(ValueError):
        _check_criterion(FusedSegLoss(ignore_index=0, focal_gamma=2.0), 255)
