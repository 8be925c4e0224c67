"""Single-scale evaluation on the HIP path: dfm_seg_predict / dfm_rows_argmax against torch, and
dformer_amd.evaluate.evaluate / save_preds / EncoderDecoder.predict against the reference's own
evaluate (utils/val_mm.py:102-207; tests/golden/eval_*.npz from oracle/golden_eval.py)."""
import functools
import os

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


class Cfg(dict):
    __getattr__ = dict.__getitem__


# (B, ncls, (h, w), (H, W))
SHAPES = [
    (2, 40, (8, 12), (64, 96)),      # x8, the ham head's factor
    (2, 37, (9, 13), (67, 101)),     # non-integer factor; W is not a multiple of any tile
    (1, 2, (15, 20), (120, 160)),    # several workgroups on both axes, two classes
    (3, 13, (5, 7), (50, 70)),
    (2, 64, (6, 8), (48, 64)),       # kMaxCls
    (1, 40, (5, 7), (5, 7)),         # identity
]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def _case(B, ncls, hw, HW, dt):
    """(low [B, ncls, h, w] in dt, fp64 argmax of its upsampling, fp64 top-2 gap, max |logit|): the
    reference sees the dtype-rounded inputs."""
    g = torch.Generator(device="cpu").manual_seed(0)
    low = torch.randn(B, ncls, *hw, generator=g).to(dt).to(DEV)
    up = F.interpolate(low.double(), size=HW, mode="bilinear", align_corners=False)
    top = up.topk(2, dim=1).values
    return low, up.argmax(1), top[:, 0] - top[:, 1], up.abs().max().item()


def _rows(low):
    return low.permute(0, 2, 3, 1).contiguous().view(-1, low.shape[1])


def _check_pred(pred, ref, gap, amax):
    """A pixel may differ from the fp64 argmax only inside the near-tie band 1e-5 * max |logit| (fp32
    interpolation of four taps errs by a few 1e-7 of the taps' magnitude), and at most 1e-3 of the
    pixels may."""
    diff = pred.long() != ref
    print(f"differing pixels {int(diff.sum())} of {diff.numel()}; in the band {int((gap <= 1e-5 * amax).sum())}")
    assert bool((gap[diff] <= 1e-5 * amax).all()), gap[diff].max().item() / amax
    assert diff.float().mean().item() <= 1e-3


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,ncls,hw,HW", SHAPES)
def test_seg_predict_vs_torch(B, ncls, hw, HW, dt):
    from dformer_amd import kernels as K
    low, ref, gap, amax = _case(B, ncls, hw, HW, dt)
    pred = K.seg_predict(_rows(low), B, hw[0], hw[1], ncls, HW)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (B, *HW)
    _check_pred(pred, ref, gap, amax)


# small factors: the staged patch times ncls exceeds the LDS budget, so the classes go through in chunks
CHUNKED = [
    (1, 64, (24, 40), (48, 80)),     # x2: 11 x 35 cells, 4 chunks of 20 classes
    (1, 40, (40, 72), (40, 72)),     # identity on more than one workgroup: 17 x 65 cells, 10 chunks of 4
    (2, 37, (30, 50), (33, 70)),     # factors 1.1 x 1.4, the last chunk partial
]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,ncls,hw,HW", CHUNKED)
def test_seg_predict_class_chunks(B, ncls, hw, HW, dt):
    from dformer_amd import kernels as K
    low, ref, gap, amax = _case(B, ncls, hw, HW, dt)
    lab = (ref + (torch.arange(ref.numel(), device=DEV).view(ref.shape) % 3 == 0)) % ncls  # a third off by one
    hist = torch.zeros(ncls * ncls, dtype=torch.int64, device=DEV)
    pred = torch.empty(B, *HW, dtype=torch.uint8, device=DEV)
    K.seg_predict(_rows(low), B, hw[0], hw[1], ncls, HW, pred=pred, label=lab, hist=hist)
    _check_pred(pred, ref, gap, amax)
    assert torch.equal(hist, torch.bincount(lab.view(-1) * ncls + pred.view(-1).long(), minlength=ncls * ncls))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
def test_seg_predict_column_slice(dt):
    """ldl = ncls + 24: the logits are a column slice of a wider buffer whose other columns are larger."""
    from dformer_amd import kernels as K
    B, ncls, hw, HW = SHAPES[1]
    low, ref, gap, amax = _case(B, ncls, hw, HW, dt)
    wide = torch.full((B * hw[0] * hw[1], ncls + 24), 100.0, device=DEV, dtype=dt)
    wide[:, 8:8 + ncls] = _rows(low)
    rows = wide[:, 8:8 + ncls]
    assert rows.stride(0) == ncls + 24
    _check_pred(K.seg_predict(rows, B, hw[0], hw[1], ncls, HW), ref, gap, amax)


def _taps(n_in, n_out):
    """PyTorch's align_corners=False source rows (i0, i1) per destination index, in float32."""
    f = np.float32
    src = np.maximum(f(n_in) / f(n_out) * (np.arange(n_out, dtype=f) + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1)


@pytest.mark.parametrize("B,ncls,hw,HW", SHAPES[:2])
def test_seg_predict_ties_go_to_the_first_class(B, ncls, hw, HW):
    from dformer_amd import kernels as K
    low = _case(B, ncls, hw, HW, torch.float32)[0].clone()
    low[:, :, :3, :] = 0.5
    pred = K.seg_predict(_rows(low), B, hw[0], hw[1], ncls, HW)
    _, i1 = _taps(hw[0], HW[0])
    tied = torch.from_numpy(i1 <= 2).to(DEV)
    assert 0 < int(tied.sum()) < HW[0]
    assert int(pred[:, tied, :].max()) == 0
    assert int(pred[:, ~tied, :].max()) > 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,ncls,hw,HW", [SHAPES[1], SHAPES[4]])
def test_seg_predict_histogram(B, ncls, hw, HW, dt):
    from dformer_amd import kernels as K
    low = _case(B, ncls, hw, HW, dt)[0]
    rows = _rows(low)
    g = torch.Generator(device="cpu").manual_seed(1)
    lab = torch.randint(0, ncls, (B, *HW), generator=g)
    lab[torch.rand(B, *HW, generator=g) < 0.1] = 255
    lab.view(-1)[:4] = torch.tensor([-1, ncls, 300, -7])  # out of range: not counted
    lab = lab.to(DEV)
    pred = torch.empty(B, *HW, dtype=torch.uint8, device=DEV)
    h1 = torch.zeros(ncls * ncls, dtype=torch.int64, device=DEV)
    h2 = torch.zeros_like(h1)
    assert K.seg_predict(rows, B, hw[0], hw[1], ncls, HW, pred=pred, label=lab, hist=h1) is pred
    assert K.seg_predict(rows, B, hw[0], hw[1], ncls, HW, label=lab, hist=h2) is h2  # the histogram alone
    keep = (lab >= 0) & (lab < ncls)  # 255 >= ncls
    want = torch.bincount(lab[keep] * ncls + pred[keep].long(), minlength=ncls * ncls)
    assert int(want.sum()) == int(keep.sum()) > 0
    assert torch.equal(h1, want) and torch.equal(h2, want)
    assert torch.equal(pred, K.seg_predict(rows, B, hw[0], hw[1], ncls, HW))
    # K.seg_confusion over torch's float32 upsampled scores: equal wherever the two argmaxes agree
    up = F.interpolate(low.float(), size=HW, mode="bilinear", align_corners=False)
    h3 = torch.zeros_like(h1)
    K.seg_confusion(up.permute(0, 2, 3, 1).contiguous().view(-1, ncls), lab, ncls, 255, h3)
    moved = int(((up.argmax(1) != pred.long()) & keep).sum())
    print(f"pixels whose float32 torch argmax differs: {moved}")
    assert int(h3.sum()) == int(h1.sum()) and int((h3 - h1).abs().sum()) // 2 <= moved
    K.seg_predict(rows, B, hw[0], hw[1], ncls, HW, label=lab, hist=h1)  # it accumulates
    assert torch.equal(h1, 2 * want)


@pytest.mark.parametrize("ncls", [1, 7, 40, 64])
def test_rows_argmax(ncls):
    from dformer_amd import kernels as K
    g = torch.Generator(device="cpu").manual_seed(2)
    acc = torch.randn(3001, ncls, generator=g)
    acc[:40] = 0.25                      # whole rows tied
    if ncls > 5:
        acc[40:80, 5] = 9.0              # ties between two lanes of a group, and within one lane
        acc[40:80, ncls - 1] = 9.0
        acc[80:120, 3] = 9.0
        acc[80:120, min(11, ncls - 1)] = 9.0
    acc = acc.to(DEV)
    out = K.rows_argmax(acc, ncls)
    assert out.dtype == torch.uint8 and torch.equal(out.long(), acc.argmax(1))


# ----------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _model(dec, ncls, embed):
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder=dec, decoder_embed_dim=embed, num_classes=ncls, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, eval_crop_size=[32, 32], eval_stride_rate=2 / 3)
    model = EncoderDecoder(cfg=cfg)
    sd = model.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    return model.cuda().eval(), cfg


def _loader(B, H, W, ncls, n=2):
    out = []
    for i in range(n):
        rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=8964 + i)
        dep = torch.from_numpy(dep_np).float()
        out.append({"rgb": torch.from_numpy(rgb_np).float(), "laser": dep, "modal_x": dep,
                    "gt": torch.from_numpy(gen.labels(B, H, W, ncls, seed=8964 + i)),
                    "fn": [f"datasets/NYU/RGB/{i}_{j}.jpg" for j in range(B)],
                    "rgb_path": [f"datasets/NYU/RGB/{i}_{j}.jpg" for j in range(B)]})
    return out


@pytest.mark.parametrize("name,dec,ncls,embed", [("eval_tiny_ham", "ham", 40, 512),
                                                 ("eval_tiny_mlp", "MLPDecoder", 37, 64)])
def test_evaluate_vs_reference_golden(name, dec, ncls, embed):
    """The HIP evaluate (fp32) against the reference's own evaluate over two batches. A pixel of
    model.predict may differ from the reference's argmax only where the float64 top-2 gap is within
    2e-3 of max |logit| (the project's fp32 gate is 1e-3 of max per logit, and two logits can move), at
    most max(2, 1e-3 * npix) pixels may, and the histogram gets test_eval_gpu.py's allowance.
    Share of pixels inside the band (oracle/golden_eval.py): eval_tiny_ham 58 of 14000 (0.41%),
    eval_tiny_mlp 226 of 14000 (1.61%)."""
    from dformer_amd.evaluate import evaluate
    g = load(name)
    B, H, W, n = [int(v) for v in g["meta"]]
    assert n == ncls
    model, cfg = _model(dec, ncls, embed)
    if dec == "ham":
        model.decode_head.hamburger.ham.injected_bases = torch.from_numpy(
            gen.nmf_bases(B, 512, 64, name=name + "/bases")).float()
    loader = _loader(B, H, W, ncls)
    amax = float(g["amax"])
    for i, batch in enumerate(loader):
        pred = model.predict(batch["rgb"].cuda(), batch["laser"].cuda()).cpu().numpy()
        assert pred.dtype == np.uint8 and pred.shape == (B, H, W)
        diff = pred != g[f"pred{i}"]
        print(f"{name} batch {i}: {int(diff.sum())} of {diff.size} pixels differ")
        assert (g[f"gap{i}"][diff] <= 2e-3 * amax).all(), g[f"gap{i}"][diff].max() / amax
        assert diff.sum() <= max(2, 1e-3 * diff.size)
    m = evaluate(model, [{k: v for k, v in b.items() if k != "modal_x"} for b in loader], cfg, DEV)
    ours, ref = m.hist.cpu().numpy(), g["hist"]
    valid = ref.sum()
    print(f"{name}: histogram distance {np.abs(ours - ref).sum() / 2} of {valid}")
    assert ours.sum() == valid
    assert np.abs(ours - ref).sum() / 2 <= max(2, 1e-3 * valid)
    ious, miou = m.compute_iou()
    f1, mf1 = m.compute_f1()
    acc, macc = m.compute_pixel_acc()
    assert len(ious) == len(f1) == len(acc) == ncls
    assert all(0.0 <= v <= 100.0 for v in (miou, mf1, macc))


@pytest.fixture(scope="module")
def ham64():
    """DFormer-Tiny + ham on two 2 x 64 x 96 batches (a multiple of 32: evaluate_msf's resizes are identities)."""
    model, cfg = _model("ham", 40, 512)
    model.decode_head.hamburger.ham.injected_bases = torch.from_numpy(gen.nmf_bases(2, 512, 64, name="eval64")).float()
    return model, cfg, _loader(2, 64, 96, 40)


def test_evaluate_matches_evaluate_msf_at_one_scale(ham64):
    from dformer_amd.evaluate import evaluate, evaluate_msf
    model, cfg, loader = ham64
    a = evaluate(model, loader, cfg, DEV).hist.cpu().numpy()
    b = evaluate_msf(model, loader, cfg, DEV, [1.0], False).hist.cpu().numpy()
    valid = b.sum()
    print(f"histogram distance {np.abs(a - b).sum() / 2} of {valid}")
    assert a.sum() == valid > 0
    assert np.abs(a - b).sum() / 2 <= max(2, 1e-3 * valid)


def test_evaluate_sliding_equals_slide_inference(ham64):
    from dformer_amd.evaluate import Metrics, evaluate, slide_inference
    model, cfg, loader = ham64
    m = evaluate(model, loader, cfg, DEV, sliding=True)
    want = Metrics(cfg.num_classes, cfg.background, DEV)
    for b in loader:
        scores = slide_inference(model, b["rgb"].cuda(), b["laser"].cuda(), cfg)
        want.update_rows(scores.permute(0, 2, 3, 1).contiguous().view(-1, cfg.num_classes), b["gt"].cuda())
    assert m.index == want.index == 2
    assert torch.equal(m._hist, want._hist) and int(m._hist.sum()) > 0


@pytest.mark.parametrize("sliding", [False, True])
def test_save_preds_writes_one_map_per_image(ham64, tmp_path, sliding):
    from dformer_amd.evaluate import evaluate, save_preds, slide_inference
    model, cfg, loader = ham64
    m = save_preds(model, loader, cfg, DEV, model_path="run", sliding=sliding, out_root=str(tmp_path))
    assert torch.equal(m._hist, evaluate(model, loader, cfg, DEV, sliding=sliding)._hist)
    assert sorted(os.listdir(tmp_path / "run")) == ["0_0.npy", "0_1.npy", "1_0.npy", "1_1.npy"]
    for i, b in enumerate(loader):
        if sliding:
            pred = slide_inference(model, b["rgb"].cuda(), b["laser"].cuda(), cfg).argmax(1).cpu().numpy()
        else:
            pred = model.predict(b["rgb"].cuda(), b["laser"].cuda()).cpu().numpy()
        for j in range(2):
            got = np.load(tmp_path / "run" / f"{i}_{j}.npy")
            assert got.dtype == np.uint8 and np.array_equal(got, pred[j])


def test_distributed_engine_returns_every_ranks_metrics(ham64, tmp_path, monkeypatch):
    """engine.distributed: a list with one Metrics per rank (here one), equal to the call without an engine."""
    from types import SimpleNamespace
    from dformer_amd.evaluate import Metrics, evaluate, evaluate_msf, save_preds
    model, cfg, loader = ham64
    gathered = []

    def all_gather_object(out, obj):
        out[0] = obj
        gathered.append(obj)

    monkeypatch.setattr(torch.distributed, "all_gather_object", all_gather_object)
    runs = {"evaluate_msf": lambda e: evaluate_msf(model, loader, cfg, DEV, [1.0], False, engine=e),
            "evaluate": lambda e: evaluate(model, loader, cfg, DEV, engine=e),
            "save_preds": lambda e: save_preds(model, loader, cfg, DEV, engine=e, model_path="run",
                                               out_root=str(tmp_path))}
    for name, run in runs.items():
        got = run(SimpleNamespace(distributed=True, world_size=1))
        assert isinstance(got, list) and len(got) == 1 and isinstance(got[0], Metrics), name
        assert got[0] is gathered[-1]
        assert torch.equal(got[0]._hist, run(None)._hist) and int(got[0]._hist.sum()) > 0, name
    assert len(gathered) == 3


def test_evaluate_save_dir_writes_pngs(ham64, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dformer_amd.evaluate import evaluate
    model, cfg, loader = ham64
    palette = np.random.RandomState(0).randint(0, 256, (41, 3)).astype(np.uint8)
    evaluate(model, loader, cfg, DEV, save_dir=str(tmp_path / "col"), palette=palette)
    evaluate(model, loader, Cfg(cfg, palette=palette.tolist()), DEV, save_dir=str(tmp_path / "cfg"))
    evaluate(model, loader, cfg, DEV, save_dir=str(tmp_path / "idx"))
    for i, b in enumerate(loader):
        pred = model.predict(b["rgb"].cuda(), b["laser"].cuda()).cpu().numpy()
        for j in range(2):
            rel = os.path.join("NYU", "RGB", f"{i}_{j}_pred.png")
            for d in ("col", "cfg"):
                img = np.array(Image.open(tmp_path / d / rel))
                assert img.shape == (64, 96, 3) and np.array_equal(img, palette[pred[j]])
            idx = np.array(Image.open(tmp_path / "idx" / rel))
            assert idx.dtype == np.uint8 and np.array_equal(idx, pred[j])


def test_evaluate_rejects_a_gt_of_another_size(ham64):
    from dformer_amd.evaluate import evaluate
    model, cfg, loader = ham64
    bad = dict(loader[0], gt=loader[0]["gt"][:, :32, :48])
    with pytest.raises(ValueError):
        evaluate(model, [bad], cfg, DEV)
    with pytest.raises(ValueError):
        evaluate(model, [bad], cfg, DEV, sliding=True)
