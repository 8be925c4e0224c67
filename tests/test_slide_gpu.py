"""Sliding-window multi-scale evaluation on the GPU (csrc/eval.hip dfm_slide_msf_accumulate,
dformer_amd.evaluate): the kernel against a torch restatement of utils/val_mm.py:257-322 + 377-397,
slide_inference against the same restatement around the model's own encode_decode, and msf_scores /
evaluate_msf with sliding windows against the reference's own run (oracle/golden_eval.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
from goldens import load

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.manual_seed(0)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def windows(n, crop, stride):
    """val_mm.py:295-306 written out again (not the package's slide_windows)."""
    grids = max(n - crop + stride - 1, 0) // stride + 1
    out = []
    for i in range(grids):
        a = i * stride
        b = min(a + crop, n)
        out.append((max(b - crop, 0), b))
    return out


def slide_restated(window_logits, B, ncls, crop, stride, scaled):
    """val_mm.py:297-319: every window's full-resolution logits (window_logits(y1, y2, x1, x2) ->
    [B, ncls, hc, wc]) zero-padded to the scaled size, summed, divided by the count map."""
    Hs, Ws = scaled
    preds = torch.zeros(B, ncls, Hs, Ws, device=DEV)
    count = torch.zeros(B, 1, Hs, Ws, device=DEV)
    for y1, y2 in windows(Hs, crop[0], stride[0]):
        for x1, x2 in windows(Ws, crop[1], stride[1]):
            preds += F.pad(window_logits(y1, y2, x1, x2), (x1, Ws - x2, y1, Hs - y2))
            count[:, :, y1:y2, x1:x2] += 1
    assert (count == 0).sum() == 0
    return preds / count


def tail_restated(logits, out_hw, flip):
    """val_mm.py:377-379 / 393-396: flip back, resize to the label size."""
    if flip:
        logits = torch.flip(logits, dims=(3,))
    return F.interpolate(logits, size=out_hw, mode="bilinear", align_corners=True)


B_, H_, W_ = 2, 5, 7
CROP, STRIDE, SCALED = (19, 23), (12, 15), (47, 52)  # 4 x 3 windows, the last row and column moved back


@functools.lru_cache(maxsize=None)
def kernel_case(ncls, dt, scaled):
    """(low [G, B, ncls, h, w] in dt, its NHWC rows, the restated averaged logits at the scaled size)."""
    G = len(windows(scaled[0], CROP[0], STRIDE[0])) * len(windows(scaled[1], CROP[1], STRIDE[1]))
    gsd = torch.Generator(device=DEV).manual_seed(1000 + ncls)
    low = torch.randn(G, B_, ncls, H_, W_, device=DEV, generator=gsd).to(dt)
    rows = low.permute(0, 1, 3, 4, 2).contiguous().view(-1, ncls)
    order = iter(range(G))

    def window_logits(y1, y2, x1, x2):
        return F.interpolate(low[next(order)].float(), size=CROP, mode="bilinear", align_corners=False)

    avg = slide_restated(window_logits, B_, ncls, CROP, STRIDE, scaled)
    return low, rows, avg


def test_kernel_case_grid():
    assert windows(47, 19, 12) == [(0, 19), (12, 31), (24, 43), (28, 47)]
    assert windows(52, 23, 15) == [(0, 23), (15, 38), (29, 52)]


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("out_hw", [(31, 45), (61, 83)])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("ncls", [13, 37, 40, 64])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_slide_msf_accumulate(dt, ncls, flip, out_hw, softmax):
    run_kernel_case(dt, ncls, flip, out_hw, softmax)


def test_slide_msf_accumulate_fp16():
    run_kernel_case(torch.float16, 40, True, (31, 45), True)


def run_kernel_case(dt, ncls, flip, out_hw, softmax):
    from dformer_amd import kernels as K
    _, rows, avg = kernel_case(ncls, dt, SCALED)
    H, W = out_hw
    acc0 = torch.rand(B_ * H * W, ncls, device=DEV)  # softmax: added to; else: overwritten
    acc = K.slide_msf_accumulate(rows, B_, H_, W_, ncls, CROP, STRIDE, SCALED, out_hw, flip, acc0.clone(),
                                 softmax=softmax)
    z = tail_restated(avg, out_hw, flip)
    ref = acc0.view(B_, H, W, ncls) + z.softmax(1).permute(0, 2, 3, 1) if softmax else z.permute(0, 2, 3, 1)
    err = rel(acc.view(B_, H, W, ncls), ref)
    print(f"slide_msf_accumulate {dt} ncls={ncls} flip={flip} out={out_hw} softmax={softmax}: rel err {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("flip", [False, True])
def test_single_window_equals_msf_accumulate(dt, flip):
    """Hs, Ws == crop: one window, and with softmax the result is msf_accumulate's on the same low (the
    same kernel: bit for bit)."""
    from dformer_amd import kernels as K
    ncls, out_hw = 40, (31, 45)
    low, rows, avg = kernel_case(ncls, dt, CROP)
    assert low.shape[0] == 1
    acc0 = torch.rand(B_ * out_hw[0] * out_hw[1], ncls, device=DEV)
    got = K.slide_msf_accumulate(rows, B_, H_, W_, ncls, CROP, STRIDE, CROP, out_hw, flip, acc0.clone())
    want = K.msf_accumulate(rows, B_, H_, W_, ncls, CROP, out_hw, flip, acc0.clone())
    assert torch.equal(got, want)
    ref = acc0.view(B_, *out_hw, ncls) + tail_restated(avg, out_hw, flip).softmax(1).permute(0, 2, 3, 1)
    assert rel(got.view(B_, *out_hw, ncls), ref) < 1e-5
    raw = K.slide_msf_accumulate(rows, B_, H_, W_, ncls, CROP, STRIDE, CROP, CROP, False, torch.empty(
        B_ * CROP[0] * CROP[1], ncls, device=DEV), softmax=False)
    assert rel(raw.view(B_, *CROP, ncls), avg.permute(0, 2, 3, 1)) < 1e-5


class Cfg(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def tiny_model(dec, ncls, embed):
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder=dec, decoder_embed_dim=embed, num_classes=ncls, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255)
    model = EncoderDecoder(cfg=cfg)
    sd = model.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    return model.cuda().eval(), cfg


def test_slide_inference_vs_restatement():
    """slide_inference (one kernel over every window's low-res logits) against the reference's composition
    around the model's own full-resolution encode_decode of each crop: 2 x 2 windows of 64 x 96."""
    from dformer_amd.evaluate import slide_inference
    model, cfg = tiny_model("MLPDecoder", 37, 64)
    cfg = Cfg(cfg, eval_crop_size=[64, 96], eval_stride_rate=0.5)
    rgb_np, dep_np = gen.rgb_depth(1, 96, 128)
    rgb, dep = torch.from_numpy(rgb_np).float().cuda(), torch.from_numpy(dep_np).float().cuda()
    with torch.no_grad():
        got = slide_inference(model, rgb, dep, cfg)
        ref = slide_restated(lambda y1, y2, x1, x2: model.encode_decode(
            rgb[:, :, y1:y2, x1:x2].contiguous(), dep[:, :, y1:y2, x1:x2].contiguous()).float(),
            1, 37, (64, 96), (32, 48), (96, 128))
    assert got.shape == (1, 37, 96, 128) and got.dtype == torch.float32
    err = rel(got, ref)
    print(f"slide_inference rel err {err:.3e}")
    assert err < 1e-4


CASES = [("slide_tiny_ham", "ham", 40, 512), ("slide_tiny_mlp", "MLPDecoder", 37, 64)]


def golden_setup(name, dec, ncls, embed):
    g = load(name)
    B, H, W, _, flip = [int(v) for v in g["meta"]]
    scores = np.stack([g["scores0_img0"]] + [load(f"{name}_img{i}")[f"scores0_img{i}"] for i in range(1, B)])
    model, cfg = tiny_model(dec, ncls, embed)
    if dec == "ham":
        model.decode_head.hamburger.ham.injected_bases = torch.from_numpy(
            gen.nmf_bases(B, 512, 64, name=name + "/bases")).float()
    loader = []
    for i in range(2):
        rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=8964 + i)
        loader.append({"rgb": torch.from_numpy(rgb_np).float(), "modal_x": torch.from_numpy(dep_np).float(),
                       "gt": torch.from_numpy(gen.labels(B, H, W, ncls, seed=8964 + i))})
    crop, rate = tuple(int(c) for c in g["crop"]), float(g["rate"])
    return g, model, cfg, loader, torch.from_numpy(scores), crop, rate, [float(s) for s in g["scales"]], bool(flip)


@pytest.mark.parametrize("name,dec,ncls,embed", CASES)
def test_msf_scores_sliding_vs_reference_golden(name, dec, ncls, embed):
    """The summed softmax scores of batch 0 against the reference's own evaluate_msf(sliding=True) at the
    project's fp32 bound, one window per model call and all windows of the largest grid in one call; the two
    chunkings agree with each other far more closely."""
    from dformer_amd import kernels as K
    from dformer_amd.evaluate import msf_scores, msf_size, slide_strides
    g, model, cfg, loader, ref, crop, rate, scales, flip = golden_setup(name, dec, ncls, embed)
    B, _, H, W = ref.shape
    strides = slide_strides(crop, rate)
    G = max(K.slide_grids(max(s[0], crop[0]), crop[0], strides[0]) *
            K.slide_grids(max(s[1], crop[1]), crop[1], strides[1]) for s in (msf_size(H, W, sc) for sc in scales))
    rgb, dep = loader[0]["rgb"].cuda(), loader[0]["modal_x"].cuda()
    got = {}
    for crop_batch in (B, G * B):
        acc = msf_scores(model, rgb, dep, ncls, scales, flip, crop_size=crop, stride_rate=rate,
                         crop_batch=crop_batch)
        got[crop_batch] = acc.view(B, H, W, ncls).permute(0, 3, 1, 2).cpu()
        err = rel(got[crop_batch], ref)
        print(f"{name} crop_batch={crop_batch}: rel err vs reference {err:.3e}")
        assert err < 1e-3, (crop_batch, err)
    both = rel(got[B], got[G * B])
    print(f"{name}: crop_batch {B} vs {G * B}: {both:.3e}")
    assert both < 1e-5, both


@pytest.mark.parametrize("name,dec,ncls,embed", CASES)
def test_evaluate_msf_sliding_vs_reference_golden(name, dec, ncls, embed):
    """evaluate_msf(sliding=True) over both batches: the confusion histogram against the reference's
    (argmax near-ties may flip a handful of pixels; the fp32 reference itself flips none)."""
    from dformer_amd.evaluate import evaluate_msf
    g, model, cfg, loader, _, crop, rate, scales, flip = golden_setup(name, dec, ncls, embed)
    cfg = Cfg(cfg, eval_crop_size=list(crop), eval_stride_rate=rate)
    m = evaluate_msf(model, loader, cfg, DEV, scales, flip, sliding=True)
    ours, ref = m.hist.cpu().numpy(), g["hist"]
    valid = ref.sum()
    diff = np.abs(ours - ref).sum() / 2
    print(f"{name}: {diff} of {valid} labelled pixels differ")
    assert ours.sum() == valid
    assert diff <= max(2, 1e-3 * valid), diff

