"""dformer_amd.data.TrainPre / ValPre (one kernel of libdformer_data.so per batch) against an fp64 oracle made of
torch ops: F.interpolate(bilinear, align_corners=False) on the mirrored source, integer indexing for the label,
slicing and F.pad for the crop and its margins.

Acceptance per image pixel (the reference's resize returns uint8, so the kernel's values sit on the grey-level
lattice): q_k = (out * std + mean) * 255 lies within 1e-3 of an integer q; q = floor(ref + 0.5), where a ref within
1e-3 of a half accepts either neighbour (the kernel interpolates in fp32: a few 1e-5 grey levels from fp64) and such
near ties must stay under 10 % of the pixels checked, so the leniency cannot hide a broken kernel; out matches
(q/255 - mean)/std in fp64 within 2e-6 (three fp32 roundings at 1/std <= 4.5 give 7e-7, doubled). Labels, padding
and the unscaled path are exact.

The raw shapes are chosen so that the oracle itself has few ties: 48 x 64 is never halved (every weight would be
exactly 1/2 and a quarter of the pixels exact ties)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MODAL_MEAN, MODAL_STD = [0.48, 0.48, 0.48], [0.28, 0.28, 0.28]
TRAV_MEAN, TRAV_STD = [0.5174, 0.4857, 0.5054], [0.2726, 0.2778, 0.2861]
SCALES = [0.5, 0.75, 1, 1.25, 1.5, 1.75]
CROPS = [(24, 40), (25, 37)]  # 37: not a multiple of the 4-pixel store width (scalar stores, a part-filled group)
PAD = float("nan")            # marks the oracle's margins


@functools.lru_cache(maxsize=None)
def raw(B, H0, W0, cm=1, seed=0):
    """Uniform random uint8 rgb [B,H0,W0,3], modal [B,H0,W0] or [B,H0,W0,3], gt [B,H0,W0] with zeros (CPU)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H0 + W0 + cm)
    rgb = torch.randint(0, 256, (B, H0, W0, 3), generator=g, dtype=torch.uint8)
    modal = torch.randint(0, 256, (B, H0, W0) + ((3,) if cm == 3 else ()), generator=g, dtype=torch.uint8)
    gt = torch.randint(0, 41, (B, H0, W0), generator=g, dtype=torch.uint8)
    assert (gt == 0).any()
    return rgb, modal, gt


def oracle_sample(img, gt, row, crop, bgr, transform_gt):
    """img [H0,W0,C] uint8, gt [H0,W0] uint8, row = (flip, sh, sw, pos_h, pos_w). Returns the grey levels before
    rounding, fp64 [C,ch,cw] with PAD in the margins, and the label int64 [ch,cw]."""
    flip, sh, sw, pos_h, pos_w = row
    ch, cw = crop
    H0, W0, C = img.shape
    if sh <= 0 or sw <= 0 or pos_h >= sh or pos_w >= sw:
        return torch.full((C, ch, cw), PAD, dtype=torch.float64), torch.full((ch, cw), 255, dtype=torch.int64)
    src = img.permute(2, 0, 1).double()[None]
    if bgr and C == 3:
        src = src.flip(1)
    if flip:
        src, gt = src.flip(-1), gt.flip(-1)  # the mirror comes first: it is applied to the source
    scaled = F.interpolate(src, size=(sh, sw), mode="bilinear", align_corners=False)[0]
    rows = torch.clamp(torch.arange(sh) * H0 // sh, max=H0 - 1)
    cols = torch.clamp(torch.arange(sw) * W0 // sw, max=W0 - 1)
    lab = gt[rows][:, cols].long()
    if transform_gt:
        lab = (lab - 1) & 255
    scaled, lab = scaled[:, pos_h:pos_h + ch, pos_w:pos_w + cw], lab[pos_h:pos_h + ch, pos_w:pos_w + cw]
    ph, pw = ch - scaled.shape[1], cw - scaled.shape[2]
    margins = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)  # the smaller half left and on top
    return F.pad(scaled, margins, value=PAD), F.pad(lab, margins, value=255)


def oracle(rgb, modal, gt, rows, crop, bgr=False, transform_gt=False):
    m3 = modal if modal.dim() == 4 else modal[..., None]
    a = [oracle_sample(rgb[b], gt[b], rows[b], crop, bgr, transform_gt) for b in range(len(rows))]
    m = [oracle_sample(m3[b], gt[b], rows[b], crop, bgr, transform_gt)[0] for b in range(len(rows))]
    return torch.stack([x[0] for x in a]), torch.stack(m), torch.stack([x[1] for x in a])


def check_image(out, ref, mean, std, exact=False):
    """out float32 [B,C,ch,cw] from the kernel, ref fp64 grey levels with PAD margins. Returns the near-tie share."""
    out = out.cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape
    C = ref.shape[1]
    m = torch.tensor(mean[:C], dtype=torch.float64).view(1, C, 1, 1)
    s = torch.tensor(std[:C], dtype=torch.float64).view(1, C, 1, 1)
    pad = ref.isnan()
    inside = ~pad
    assert (out[pad] == 0).all(), "margins must be 0.0"
    if not inside.any():
        return 0.0
    o = out.double()
    qk = (o * s + m) * 255
    q = qk.round()
    off = (qk - q).abs()[inside].max().item()
    lo = torch.floor(ref)
    near = ((ref - lo) - 0.5).abs() < 1e-3
    want = torch.floor(ref + 0.5)
    ok = (q == want) | (near & ((q == lo) | (q == lo + 1)))
    share = near[inside].double().mean().item()
    err = (o - (q / 255 - m) / s).abs()[inside].max().item()
    print(f"lattice offset {off:.2e}, wrong grey levels {int((~ok)[inside].sum())} of {int(inside.sum())}, "
          f"near ties {share:.4f}, value error {err:.2e}")
    assert off < 1e-3
    assert ok[inside].all()
    assert share < 0.10
    assert err <= 2e-6
    if exact:
        assert share == 0.0 and (q == ref)[inside].all()
    return share


def run_and_check(pre, raws, rows, crop, *, mean=MEAN, std=STD, mmean=MODAL_MEAN, mstd=MODAL_STD, exact=False,
                  device_params=False):
    rgb, modal, gt = raws
    params = torch.tensor([list(r) + [0, 0, 0] for r in rows], dtype=torch.int32)
    out = pre(rgb.to(DEV), modal.to(DEV), gt.to(DEV), params.to(DEV) if device_params else params)
    ref_rgb, ref_modal, ref_lab = oracle(rgb, modal, gt, rows, crop, pre.bgr, pre.transform_gt)
    check_image(out[0], ref_rgb, mean, std, exact)
    check_image(out[1], ref_modal, mmean, mstd, exact)
    assert out[2].dtype == torch.int64 and torch.equal(out[2].cpu(), ref_lab)
    return out


def train_pre(crop, **kw):
    from dformer_amd.data import TrainPre
    return TrainPre(kw.pop("mean", MEAN), kw.pop("std", STD), crop, SCALES, kw.pop("mmean", MODAL_MEAN),
                    kw.pop("mstd", MODAL_STD), **kw)


def centred(sh, sw, crop):
    return ((sh - crop[0] + 1) // 3 if sh > crop[0] else 0), ((sw - crop[1] + 1) // 3 if sw > crop[1] else 0)


def test_identity():
    """ValPre is normalisation only, exactly; TrainPre at scale 1 with the crop of the raw size is the same call."""
    from dformer_amd.data import TrainPre, ValPre
    raws = raw(2, 48, 64)
    val = ValPre(MEAN, STD, MODAL_MEAN, MODAL_STD)
    dev = [t.to(DEV) for t in raws]
    out = val(*dev)
    ref = oracle(*raws, [(0, 48, 64, 0, 0)] * 2, (48, 64))
    check_image(out[0], ref[0], MEAN, STD, exact=True)
    check_image(out[1], ref[1], MODAL_MEAN, MODAL_STD, exact=True)
    assert torch.equal(out[2].cpu(), raws[2].long())
    pre = TrainPre(MEAN, STD, (48, 64), None, MODAL_MEAN, MODAL_STD)
    params = pre.draw(2, (48, 64), __import__("random").Random(3))
    assert params.is_pinned() and [r[1:5] for r in params.tolist()] == [[48, 64, 0, 0]] * 2
    same = pre(*dev, torch.tensor([[0, 48, 64, 0, 0, 0, 0, 0]] * 2, dtype=torch.int32))
    assert all(torch.equal(a, b) for a, b in zip(out, same))
    # odd raw size: the rows of the outputs are not 16-byte aligned
    raws = raw(2, 23, 37)
    out = ValPre(MEAN, STD, MODAL_MEAN, MODAL_STD)(*[t.to(DEV) for t in raws])
    ref = oracle(*raws, [(0, 23, 37, 0, 0)] * 2, (23, 37))
    check_image(out[0], ref[0], MEAN, STD, exact=True)
    assert torch.equal(out[2].cpu(), raws[2].long())


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_scales(scale, flip):
    """Every scale of the reference's train_scale_array, mirrored or not, on an odd raw size, both crops. At 0.5 and
    0.75 the scaled image is smaller than a crop in one or both dimensions, from 1.25 on it is larger in both."""
    H0, W0 = 31, 45
    sh, sw = int(H0 * scale), int(W0 * scale)
    for crop in CROPS:
        run_and_check(train_pre(crop), raw(2, H0, W0), [(flip, sh, sw) + centred(sh, sw, crop)] * 2, crop,
                      exact=scale == 1)


def test_small_image_odd_pad():
    """Half of 23 x 37 is 11 x 18, smaller than both crops in both dimensions: 24 - 11 = 13 rows of padding put 6
    on top and 7 below, 37 - 18 = 19 columns put 9 on the left and 10 on the right."""
    for crop in CROPS:
        for flip in (0, 1):
            out = run_and_check(train_pre(crop), raw(2, 23, 37), [(flip, 11, 18, 0, 0)] * 2, crop)
            top, left = (crop[0] - 11) // 2, (crop[1] - 18) // 2
            lab = out[2].cpu()
            assert (lab[:, :top] == 255).all() and (lab[:, top + 11:] == 255).all() and (lab[:, :, :left] == 255).all()
            assert (lab[:, top:top + 11, left:left + 18] <= 40).all()
            assert (out[0][:, :, top + 11:] == 0).all() and (out[0][:, :, :, left + 18:] == 0).all()


def test_randint_quirk():
    """random.randint includes its upper end: pos = scaled - crop + 1 leaves the crop one row and one column
    short, padded at the bottom and on the right (1 // 2 = 0 rows on top)."""
    H0, W0 = 31, 45
    sh, sw = int(H0 * 1.5), int(W0 * 1.5)
    for crop in CROPS:
        rows = [(0, sh, sw, sh - crop[0] + 1, sw - crop[1] + 1), (1, sh, sw, sh - crop[0] + 1, 2)]
        out = run_and_check(train_pre(crop), raw(2, H0, W0), rows, crop)
        lab = out[2].cpu()
        assert (lab[:, -1] == 255).all() and (lab[0, :, -1] == 255).all() and (lab[:, :-1, :-1] <= 40).all()
        assert (lab[1, :-1, -1] <= 40).all()


def test_batch_of_three():
    """Three samples with three parameter rows in one launch (more than one block per sample at 48 x 64 crops)."""
    rows = [(1, 60, 80, 7, 11), (0, 84, 112, 84 - 48 + 1, 30), (1, 48, 64, 0, 0)]
    run_and_check(train_pre((48, 64)), raw(3, 48, 64), rows, (48, 64))
    rows = [(0, 60, 80, 30, 40), (1, 84, 112, 5, 112 - 37 + 1), (1, 48, 64, 11, 13)]
    run_and_check(train_pre((25, 37)), raw(3, 48, 64), rows, (25, 37))


def test_modal_three_channels():
    for crop in CROPS:
        run_and_check(train_pre(crop), raw(2, 23, 37, cm=3), [(1, 28, 46, 2, 5), (0, 40, 64, 9, 20)], crop)


@pytest.mark.parametrize("opts", [dict(bgr=True), dict(transform_gt=True), dict(mean=TRAV_MEAN, std=TRAV_STD),
                                  dict(bgr=True, transform_gt=True, mean=TRAV_MEAN, std=TRAV_STD, mmean=[0.4, 0.5, 0.6],
                                       mstd=[0.3, 0.25, 0.35], cm=3)],
                         ids=["bgr", "transform_gt", "trav_norm", "all_three_channel_modal"])
def test_options(opts):
    """bgr reads the source channels in reverse order; transform_gt stores (g - 1) & 255, so label 0 becomes 255;
    the Trav dataset's mean and std; all of them on a 3-channel modal with per-channel statistics."""
    opts = dict(opts)
    raws = raw(2, 31, 45, cm=opts.pop("cm", 1))
    chk = {k: opts[k] for k in ("mean", "std", "mmean", "mstd") if k in opts}
    for crop in CROPS:
        out = run_and_check(train_pre(crop, **opts), raws, [(0, 38, 56, 3, 7), (1, 23, 33, 0, 0)], crop, **chk)
        if opts.get("transform_gt"):
            lab = out[2].cpu()
            assert (lab == 255).any() and not (lab == 0).all() and ((lab <= 39) | (lab == 255)).all()
    if opts.get("bgr") and "mean" not in opts:
        plain = train_pre((24, 40))(raws[0].flip(-1).contiguous().to(DEV), raws[1].to(DEV), raws[2].to(DEV),
                                    torch.tensor([[0, 38, 56, 3, 7, 0, 0, 0]] * 2, dtype=torch.int32))
        swapped = train_pre((24, 40), bgr=True)(raws[0].to(DEV), raws[1].to(DEV), raws[2].to(DEV),
                                                torch.tensor([[0, 38, 56, 3, 7, 0, 0, 0]] * 2, dtype=torch.int32))
        assert torch.equal(plain[0], swapped[0])


def test_out_in_place():
    """out= writes the caller's tensors (a model's static input buffers) and returns them."""
    crop = (24, 40)
    raws = raw(2, 31, 45)
    dev = [t.to(DEV) for t in raws]
    params = torch.tensor([[1, 46, 67, 4, 9, 0, 0, 0], [0, 31, 45, 2, 1, 0, 0, 0]], dtype=torch.int32)
    pre = train_pre(crop)
    fresh = pre(*dev, params)
    bufs = (torch.full((2, 3, 24, 40), 7.0, device=DEV), torch.full((2, 1, 24, 40), 7.0, device=DEV),
            torch.full((2, 24, 40), 7, dtype=torch.int64, device=DEV))
    ptrs = [t.data_ptr() for t in bufs]
    got = pre(*dev, params, out=bufs)
    assert all(g is b for g, b in zip(got, bufs)) and [t.data_ptr() for t in bufs] == ptrs
    assert all(torch.equal(a, b) for a, b in zip(fresh, bufs))
    with pytest.raises(ValueError, match="out modal"):
        pre(*dev, params, out=(bufs[0], bufs[0], bufs[2]))
    with pytest.raises(ValueError, match="one raw size"):
        pre(dev[0], dev[1][:, :30].contiguous(), dev[2], params)


def test_unchecked_device_params_are_safe():
    """Device params are never read on the host, so the kernel bounds everything itself: rows that describe no
    image give padding only, and a negative position reads the first row / column (the upscaled image's first row
    and column are the source's own, so the oracle is the replicate-padded scaled image)."""
    crop = (24, 40)
    raws = raw(3, 31, 45)
    rows = [(0, 0, 56, 0, 0), (1, 38, -56, 0, 0), (0, 38, 56, 38, 0)]
    out = run_and_check(train_pre(crop), raws, rows, crop, device_params=True)
    assert (out[0] == 0).all() and (out[1] == 0).all() and (out[2] == 255).all()
    params = torch.tensor([[0, 32769, 56, 0, 0, 0, 0, 0], [0, 38, 1 << 30, 0, 0, 0, 0, 0],
                           [1, 38, 56, 0, 56, 0, 0, 0]], dtype=torch.int32, device=DEV)
    out = train_pre(crop)(*[t.to(DEV) for t in raws], params)
    assert (out[0] == 0).all() and (out[1] == 0).all() and (out[2] == 255).all()
    # pos = (-2, -3) at scale 1.25: shift the oracle's crop window by replicate-padding the scaled image
    rgb, modal, gt = raws
    big = (38 + 2, 56 + 3)
    ref = oracle(rgb, modal, gt, [(0, 38, 56, 0, 0)] * 3, (38, 56))
    ref_rgb = F.pad(ref[0], (3, 0, 2, 0), mode="replicate")[:, :, :24, :40]
    ref_lab = F.pad(ref[2].double()[:, None], (3, 0, 2, 0), mode="replicate")[:, 0, :24, :40].long()
    assert big[0] >= 24 and big[1] >= 40
    params = torch.tensor([[0, 38, 56, -2, -3, 0, 0, 0]] * 3, dtype=torch.int32, device=DEV)
    out = train_pre(crop)(*[t.to(DEV) for t in raws], params)
    check_image(out[0], ref_rgb, MEAN, STD)
    assert torch.equal(out[2].cpu(), ref_lab)


def test_graph_replay():
    """Device params make the call capturable: one linear torch.cuda.graph capture, replayed after the params and
    the raw tensors were changed in place; the static outputs follow."""
    crop = (24, 40)
    pre = train_pre(crop)
    first, second = raw(2, 31, 45), raw(2, 31, 45, seed=1)
    rows1 = [(0, 46, 67, 5, 6), (1, 31, 45, 3, 2)]
    rows2 = [(1, 54, 78, 54 - 24 + 1, 17), (0, 15, 22, 0, 0)]
    dev = [t.to(DEV) for t in first]
    params = torch.tensor([list(r) + [0, 0, 0] for r in rows1], dtype=torch.int32, device=DEV)
    bufs = (torch.empty(2, 3, 24, 40, device=DEV), torch.empty(2, 1, 24, 40, device=DEV),
            torch.empty(2, 24, 40, dtype=torch.int64, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pre(*dev, params, out=bufs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pre(*dev, params, out=bufs)
    for t in bufs:
        t.zero_()
    graph.replay()
    ref = oracle(*first, rows1, crop)
    check_image(bufs[0], ref[0], MEAN, STD)
    check_image(bufs[1], ref[1], MODAL_MEAN, MODAL_STD)
    assert torch.equal(bufs[2].cpu(), ref[2])
    for d, s in zip(dev, second):
        d.copy_(s)
    params.copy_(torch.tensor([list(r) + [0, 0, 0] for r in rows2], dtype=torch.int32))
    graph.replay()
    ref2 = oracle(*second, rows2, crop)
    check_image(bufs[0], ref2[0], MEAN, STD)
    check_image(bufs[1], ref2[1], MODAL_MEAN, MODAL_STD)
    assert torch.equal(bufs[2].cpu(), ref2[2])
    assert not torch.equal(ref[2], ref2[2])
