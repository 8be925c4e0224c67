"""Single-scale evaluation and prediction export, the parts that need no GPU: argument validation of
dfm_seg_predict / dfm_rows_argmax, the declarations, the host-side naming and palette helpers, and the
self-consistency of the reference fixtures (oracle/golden_eval.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gen
from goldens import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20  # an address that is never dereferenced: validation fails first

GOOD = dict(dtype=0, B=2, h=5, w=7, ncls=40, low=FAKE, ldl=40, H=40, W=56, pred=FAKE, label=FAKE, ignore=255,
            hist=FAKE, stream=None)


@pytest.mark.parametrize("bad,says", [
    (dict(low=None), b"null pointer"),
    (dict(ncls=0), b"ncls=0"), (dict(ncls=65), b"ncls=65"),
    (dict(H=4), b"exceeds the output"), (dict(W=6), b"exceeds the output"),
    (dict(pred=None, label=None, hist=None), b"no output"),
    (dict(hist=None), b"go together"), (dict(pred=None, hist=None), b"go together"),
    (dict(label=None), b"go together"),
    (dict(ldl=39), b"bad argument"), (dict(B=0), b"bad argument"), (dict(h=0), b"bad argument"),
    (dict(W=0), b"bad argument")])
def test_seg_predict_rejects_bad_arguments(bad, says):
    """Status -1 and a message that names the entry point and the defect, before anything touches the GPU."""
    from dformer_amd import _lib
    a = dict(GOOD)
    a.update(bad)
    st = _lib.lib.dfm_seg_predict(*a.values())
    err = _lib.lib.dfm_last_error()
    assert st == -1, (bad, st, err)
    assert err.startswith(b"dfm_seg_predict: ") and says in err, err


def test_seg_predict_rejects_unknown_dtype_first():
    from dformer_amd import _lib
    res, argtypes = _lib._SIGS["dfm_seg_predict"]
    assert res is ctypes.c_int and len(argtypes) == 14
    args = [0 if t in (ctypes.c_int, ctypes.c_long) else None for t in argtypes]
    args[0] = 7
    assert _lib.lib.dfm_seg_predict(*args) == -2
    assert b"dfm_seg_predict: unsupported dtype 7" in _lib.lib.dfm_last_error()
    assert _lib.lib.dfm_abi_version() == 13 == _lib.ABI_VERSION  # new symbols, no layout change


@pytest.mark.parametrize("args,says", [
    ((10, 40, None, FAKE, None), b"null pointer"), ((10, 40, FAKE, None, None), b"null pointer"),
    ((10, 0, FAKE, FAKE, None), b"ncls=0"), ((10, 65, FAKE, FAKE, None), b"ncls=65"),
    ((-1, 40, FAKE, FAKE, None), b"bad argument")])
def test_rows_argmax_rejects_bad_arguments(args, says):
    from dformer_amd import _lib
    st = _lib.lib.dfm_rows_argmax(*args)
    err = _lib.lib.dfm_last_error()
    assert st == -1, (args, st, err)
    assert err.startswith(b"dfm_rows_argmax: ") and says in err, err


def test_symbols_declared_everywhere():
    """Header, library and _SIGS agree on the two new entry points (argument counts included)."""
    from dformer_amd import _lib
    text = open(os.path.join(ROOT, "include", "dformer_hip.h")).read()
    for name in ("dfm_seg_predict", "dfm_rows_argmax"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib._SIGS[name][1])
        assert name in _lib.SYMBOLS and hasattr(_lib.lib, name)


def test_python_wrappers_check_buffers():
    from dformer_amd import kernels as K
    B, h, w, ncls, H, W = 2, 5, 7, 13, 40, 56
    low = torch.zeros(B * h * w, ncls)
    lab = torch.zeros(B, H, W, dtype=torch.int64)
    hist = torch.zeros(ncls * ncls, dtype=torch.int64)
    with pytest.raises(ValueError):  # a batch short
        K.seg_predict(low[:-1], B, h, w, ncls, (H, W))
    with pytest.raises(ValueError):  # fewer columns than classes
        K.seg_predict(low, B, h, w, ncls + 1, (H, W))
    with pytest.raises(ValueError):  # label without hist
        K.seg_predict(low, B, h, w, ncls, (H, W), label=lab)
    with pytest.raises(ValueError):  # label of another size
        K.seg_predict(low, B, h, w, ncls, (H, W + 1), label=lab, hist=hist)
    with pytest.raises(ValueError):  # int32 labels
        K.seg_predict(low, B, h, w, ncls, (H, W), label=lab.int(), hist=hist)
    with pytest.raises(ValueError):  # hist of another size
        K.seg_predict(low, B, h, w, ncls, (H, W), label=lab, hist=hist[:-1])
    with pytest.raises(ValueError):  # pred of another dtype
        K.seg_predict(low, B, h, w, ncls, (H, W), pred=torch.zeros(B, H, W, dtype=torch.int32))
    with pytest.raises(ValueError):
        K.rows_argmax(torch.zeros(10, ncls), ncls + 1)
    with pytest.raises(ValueError):
        K.rows_argmax(torch.zeros(10, ncls, dtype=torch.float64), ncls)
    with pytest.raises(ValueError):
        K.rows_argmax(torch.zeros(10, ncls), ncls, out=torch.zeros(9, dtype=torch.uint8))


def test_export_names():
    from dformer_amd.evaluate import pred_img_id, pred_png_name
    assert pred_png_name("datasets/NYUDepthv2/RGB/12.jpg") == "NYUDepthv2/RGB/12"
    assert pred_png_name("RGB/a.png") == "RGB/a" and pred_png_name("x") == "x"
    assert pred_png_name("a.jpg.png") == "a"  # every occurrence goes, like str.replace
    # str.strip('.jpg') strips the characters '.', 'j', 'p', 'g' from both ends, not the suffix
    assert pred_img_id("datasets/NYUDepthv2/RGB/123.jpg") == "123"
    assert pred_img_id("a/b/great_pig.jpg") == "reat_pi"
    assert pred_img_id("a/b/great_pig.jpg") == "great_pig.jpg".strip(".jpg")
    assert pred_img_id("plain.png") == "lain.pn"
    assert pred_img_id("no_dir.jpg") == "no_dir"


def test_palette_validation():
    from dformer_amd.evaluate import check_palette
    pal = np.arange(40 * 3).reshape(40, 3) % 256
    out = check_palette(pal, 40)
    assert out.dtype == np.uint8 and out.shape == (40, 3) and np.array_equal(out, pal)
    assert check_palette(torch.from_numpy(pal.astype(np.uint8)), 37).shape == (40, 3)  # more rows than classes
    assert check_palette(pal.tolist(), 40).dtype == np.uint8
    for bad in (pal[:39], pal[:, :2], pal.reshape(-1), pal + 200, pal.astype(np.float32) / 255, -pal):
        with pytest.raises(ValueError):
            check_palette(bad, 40)


def test_gt_size_mismatch_raises_before_the_model():
    from dformer_amd.evaluate import evaluate

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    class Model:
        def eval(self):
            return self

    batch = {"rgb": torch.zeros(3, 32, 32), "laser": torch.zeros(3, 32, 32), "gt": torch.zeros(16, 16)}
    with pytest.raises(ValueError, match="do not match the image"):
        evaluate(Model(), [batch], Cfg(num_classes=4, background=255), "cpu")
    with pytest.raises(ValueError):  # a bad sliding stride fails before the first batch
        evaluate(None, [], Cfg(num_classes=4, background=255, eval_crop_size=[32, 32], eval_stride_rate=0.0), "cpu",
                 sliding=True)


def test_bad_stride_rate_raises_before_the_first_batch(tmp_path):
    """sliding=True with a stride of int(0 * crop) = 0: every entry point raises before it iterates."""
    from dformer_amd.evaluate import evaluate, evaluate_msf, save_preds

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    class Model:
        def eval(self):
            return self

    class Loader:
        def __iter__(self):
            raise AssertionError("the dataloader was touched")

    cfg = Cfg(num_classes=4, background=255, eval_crop_size=[32, 32], eval_stride_rate=0.0)
    with pytest.raises(ValueError, match="must be positive"):
        evaluate_msf(Model(), Loader(), cfg, "cpu", [1.0], False, sliding=True)
    with pytest.raises(ValueError, match="must be positive"):
        evaluate(Model(), Loader(), cfg, "cpu", sliding=True)
    with pytest.raises(ValueError, match="must be positive"):
        save_preds(Model(), Loader(), cfg, "cpu", model_path="run", sliding=True, out_root=str(tmp_path))
    with pytest.raises(AssertionError, match="touched"):  # a good rate gets as far as the loader
        evaluate(Model(), Loader(), Cfg(cfg, eval_stride_rate=0.5), "cpu", sliding=True)


@pytest.mark.parametrize("name,ncls", [("eval_tiny_ham", 40), ("eval_tiny_mlp", 37)])
def test_fixture_is_self_consistent(name, ncls):
    """hist of the reference's evaluate == bincount over its own argmax maps and gen's labels."""
    g = load(name)
    B, H, W, n = [int(v) for v in g["meta"]]
    assert (B, H, W, n) == (2, 50, 70, ncls)
    want = np.zeros(ncls * ncls, dtype=np.int64)
    for i in range(2):
        lab = gen.labels(B, H, W, ncls, seed=8964 + i)
        pred, gap = g[f"pred{i}"], g[f"gap{i}"]
        assert pred.dtype == np.uint8 and pred.shape == (B, H, W) and pred.max() < ncls
        assert gap.dtype == np.float32 and gap.shape == (B, H, W) and gap.min() >= 0
        keep = (lab != 255) & (lab >= 0) & (lab < ncls)
        want += np.bincount(lab[keep].astype(np.int64) * ncls + pred[keep], minlength=ncls * ncls)
    assert np.array_equal(g["hist"].astype(np.int64).reshape(-1), want)
    assert 0 < float(g["amax"]) < 10
