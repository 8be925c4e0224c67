"""Sliding-window evaluation, the parts that need no GPU: the window rule (utils/val_mm.py:295-306)
against the windows the reference used, argument validation of dfm_slide_msf_accumulate, and the
tiling of injected NMF bases over a stack of crops."""
import ctypes

import pytest
import torch

from goldens import load


@pytest.mark.parametrize("name", ["slide_tiny_ham", "slide_tiny_mlp"])
def test_slide_windows_match_reference(name):
    """slide_windows on the size each scale was cut from equals the windows the reference padded its crop
    logits back into (oracle/golden_eval.py), per scale and axis."""
    from dformer_amd.evaluate import msf_size, slide_strides, slide_windows
    g = load(name)
    _, H, W, _, _ = [int(v) for v in g["meta"]]
    crop = tuple(int(c) for c in g["crop"])
    strides = slide_strides(crop, float(g["rate"]))
    for k, scale in enumerate(g["scales"]):
        Hs, Ws = msf_size(H, W, float(scale))
        if crop[0] > Hs or crop[1] > Ws:  # val_mm.py:280-286: both dimensions become the crop's
            Hs, Ws = crop
        assert (Hs, Ws) == tuple(int(v) for v in g[f"size{k}"])
        assert slide_windows(Hs, crop[0], strides[0]) == [tuple(int(v) for v in r) for r in g[f"win_h{k}"]]
        assert slide_windows(Ws, crop[1], strides[1]) == [tuple(int(v) for v in r) for r in g[f"win_w{k}"]]


def test_fixture_window_grids():
    """The fixtures cover what they were chosen for: 1x2, 2x2 and 3x4 grids with clamped last windows
    (ham), two up-sized scales and a 2x2 grid (mlp)."""
    g = load("slide_tiny_ham")
    assert [(len(g[f"win_h{k}"]), len(g[f"win_w{k}"])) for k in range(3)] == [(1, 2), (2, 2), (3, 4)]
    stride = int(2 / 3 * 64)
    assert g["win_h2"][-1][0] < 2 * stride and g["win_w2"][-1][0] < 3 * stride  # moved back to end at n
    m = load("slide_tiny_mlp")
    assert [tuple(m[f"size{k}"]) for k in range(2)] == [(64, 96), (64, 96)]
    assert [(len(m[f"win_h{k}"]), len(m[f"win_w{k}"])) for k in range(3)] == [(1, 1), (1, 1), (2, 2)]


def test_slide_windows_hand_cases():
    from dformer_amd.evaluate import slide_windows
    assert slide_windows(64, 64, 42) == [(0, 64)]                       # n == crop: one window
    assert slide_windows(10, 4, 3) == [(0, 4), (3, 7), (6, 10)]         # (n - crop) % stride == 0: no duplicate
    assert slide_windows(11, 4, 3) == [(0, 4), (3, 7), (6, 10), (7, 11)]  # the last window moved back
    assert slide_windows(10, 3, 5) == [(0, 3), (5, 8), (7, 10)]         # stride > crop
    assert slide_windows(96, 64, 42) == [(0, 64), (32, 96)]
    assert slide_windows(3, 4, 2) == [(0, 3)]                           # smaller than the crop: start clamped to 0


def test_zero_stride_raises():
    from dformer_amd.evaluate import msf_scores, slide_inference, slide_strides
    with pytest.raises(ValueError):
        slide_strides((64, 64), 0.01)  # int(0.64) == 0
    with pytest.raises(ValueError):
        slide_strides((64, 1), 0.5)    # one axis is enough
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(ValueError):    # before any model or GPU work
        msf_scores(None, img, img, 4, [1.0], False, crop_size=(32, 32), stride_rate=0.01)

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    with pytest.raises(ValueError):
        slide_inference(None, img, img, Cfg(eval_crop_size=(32, 32), eval_stride_rate=0.0, num_classes=4))
    assert slide_strides((480, 480), 2 / 3) == (320, 320) and slide_strides((64, 96), 0.5) == (32, 48)


GOOD = dict(dtype=0, B=2, h=5, w=7, ncls=40, low=None, ldl=40, hc=19, wc=23, hstride=12, wstride=15, Hs=47, Ws=52,
            H=31, W=45, flip=0, softmax=1, acc=None, stream=None)
FAKE = 1 << 20  # an address that is never dereferenced: validation fails first


@pytest.mark.parametrize("low,acc", [(None, None), (FAKE, None), (None, FAKE)])
def test_slide_msf_accumulate_rejects_null_pointers(low, acc):
    """Well-formed shapes with a null pointer: status -1 before anything touches the GPU."""
    from dformer_amd import _lib
    a = dict(GOOD, low=low, acc=acc)
    assert _lib.lib.dfm_slide_msf_accumulate(*a.values()) == -1
    err = _lib.lib.dfm_last_error()
    assert err.startswith(b"dfm_slide_msf_accumulate: ") and b"null pointer" in err, err


@pytest.mark.parametrize("bad,says", [
    (dict(ncls=0), b"ncls=0"), (dict(ncls=65), b"ncls=65"),
    (dict(hstride=0), b"must be positive"), (dict(wstride=-1), b"must be positive"),
    (dict(Hs=18), b"smaller than the crop"), (dict(Ws=22), b"smaller than the crop"), (dict(ldl=39), b"bad argument"),
    (dict(B=0), b"bad argument"), (dict(h=0), b"bad argument"), (dict(H=0), b"bad argument"),
    (dict(hstride=20), b"exceeds the crop"), (dict(wstride=24), b"exceeds the crop")])
def test_slide_msf_accumulate_rejects_bad_arguments(bad, says):
    """Each shape defect is rejected before any launch, with status -1 and a message that names the entry
    point and the defect: with null pointers (whatever the message), and with the pointers set (the
    test_abi.py pattern: addresses that are never dereferenced), where the message is the defect's own."""
    from dformer_amd import _lib
    a = dict(GOOD)
    a.update(bad)
    assert _lib.lib.dfm_slide_msf_accumulate(*a.values()) == -1
    a.update(low=FAKE, acc=FAKE)
    st = _lib.lib.dfm_slide_msf_accumulate(*a.values())
    err = _lib.lib.dfm_last_error()
    assert st == -1, (bad, st, err)
    assert err.startswith(b"dfm_slide_msf_accumulate: ") and says in err, err


def test_slide_msf_accumulate_null_pointer_wins_nothing_over_dtype():
    """An unknown dtype code is rejected first, like every other entry point (test_abi.py)."""
    from dformer_amd import _lib
    res, argtypes = _lib._SIGS["dfm_slide_msf_accumulate"]
    assert res is ctypes.c_int and len(argtypes) == 19
    args = [0 if t in (ctypes.c_int, ctypes.c_long) else None for t in argtypes]
    args[0] = 7
    assert _lib.lib.dfm_slide_msf_accumulate(*args) == -2
    assert b"dfm_slide_msf_accumulate: unsupported dtype 7" in _lib.lib.dfm_last_error()
    assert _lib.lib.dfm_abi_version() == 13 == _lib.ABI_VERSION  # a new symbol, no layout change


def test_python_wrapper_checks_buffer_sizes():
    """K.slide_msf_accumulate knows the buffers' sizes and refuses ones the kernel would overrun."""
    from dformer_amd import kernels as K
    B, h, w, ncls = 2, 5, 7, 13
    G = K.slide_grids(47, 19, 12) * K.slide_grids(52, 23, 15)
    assert G == 12
    acc = torch.zeros(B * 31 * 45, ncls)
    with pytest.raises(ValueError):  # one window's rows short
        K.slide_msf_accumulate(torch.zeros((G - 1) * B * h * w, ncls), B, h, w, ncls, (19, 23), (12, 15), (47, 52),
                               (31, 45), False, acc)
    with pytest.raises(ValueError):  # acc of another size
        K.slide_msf_accumulate(torch.zeros(G * B * h * w, ncls), B, h, w, ncls, (19, 23), (12, 15), (47, 52),
                               (31, 46), False, acc)


def test_injected_bases_tile_over_stacked_crops():
    """Injected bases of batch b0 serve a stack of k*b0 images: image g*b0 + i gets bases[i]; a matching
    batch gets them unchanged."""
    from dformer_amd.decoders import NMF2D
    ham = NMF2D()
    b0, D = 2, 8
    bases = torch.arange(b0 * D * ham.R, dtype=torch.float32).view(b0, D, ham.R)
    ham.injected_bases = bases
    same = ham._build_bases(b0, D, "cpu")
    assert same.shape == bases.shape and torch.equal(same, bases)
    tiled = ham._build_bases(3 * b0, D, "cpu")
    assert tiled.shape == (3 * b0, D, ham.R)
    for g in range(3):
        for i in range(b0):
            assert torch.equal(tiled[g * b0 + i], bases[i])


def test_save_dir_still_raises():
    """Prediction PNG export stays outside the path, with or without sliding windows."""
    from dformer_amd.evaluate import evaluate_msf

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    cfg = Cfg(num_classes=4, background=255, eval_crop_size=[32, 32], eval_stride_rate=0.5)
    for sliding in (False, True):
        with pytest.raises(NotImplementedError):
            evaluate_msf(None, [], cfg, "cpu", [1.0], False, save_dir="x", sliding=sliding)
