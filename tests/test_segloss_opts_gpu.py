"""Criterion options of the fused segmentation loss on the GPU (csrc/loss.hip: dfm_seg_loss_opts_*,
dfm_seg_loss_ohem_relabel; decoders.SegLossFn; losses.FusedSegLoss in EncoderDecoder): class weights and label
smoothing (builder.py:230 with nn.CrossEntropyLoss's weight= / label_smoothing=) and online hard example
mining (utils/loss_opr.py:137-187). Every oracle is written here from torch primitives on the stored logits."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (B, h, w, H, W, ncls), one per code path, the smallest with interior tiles, edge clamps and a partial block
SHAPES = [(2, 5, 7, 40, 56, 40),   # S=8 fused, 16-byte class rows
          (2, 6, 5, 24, 20, 37),   # S=4 fused, scalar class loads, 40-wide template
          (2, 7, 9, 28, 36, 64),   # S=4, 64-wide template
          (2, 4, 6, 8, 12, 64),    # S=2, tile backward only
          (1, 7, 9, 30, 41, 19),   # non-integer factor, x / y passes
          (2, 5, 7, 40, 56, 2)]    # the Trav head
OHEM_SHAPES = [s for s in SHAPES if s[0] * s[3] * s[4] * 0.9 >= 800]  # the 8 x 12 plane is too small (below)
IGNORE = 255
# tolerances of this kernel family (test_kernels_gpu.py::test_seg_loss, test_seg_loss_fwd_grad_fused)
LOSS_RTOL, GRAD_TOL, GRAD_TOL16 = 1e-4, 1e-3, 4e-3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def K():
    from dformer_amd import kernels
    return kernels


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """(logits [B, h, w, ncls] in dt, labels with 10 % ignored, weights U(0.5, 2) with one class at 0),
    generated on the CPU so a case is the same on every device; shared by the tests, never modified."""
    B, h, w, H, W, ncls = shape
    g = torch.Generator().manual_seed(1000 * h + ncls)
    lg = (3 * torch.randn(B, h, w, ncls, generator=g)).to(dt)
    lab = torch.randint(0, ncls, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    weight = 0.5 + 1.5 * torch.rand(ncls, generator=g)
    weight[ncls // 2] = 0.0
    return lg.to(DEV), lab.to(DEV), weight.to(DEV)


def torch_loss(lg, lab, weight, eps, scale=1.0):
    """F.interpolate + F.cross_entropy in fp32 on the stored logits -> (loss, scale * d loss / d logits NCHW);
    the mean is over the valid-pixel count."""
    H, W = lab.shape[-2:]
    lr = lg.float().permute(0, 3, 1, 2).contiguous().requires_grad_()
    up = F.interpolate(lr, (H, W), mode="bilinear", align_corners=False)
    ce = F.cross_entropy(up, lab, weight=weight, reduction="none", ignore_index=IGNORE, label_smoothing=eps)
    loss = ce.sum() / (lab != IGNORE).sum().clamp_min(1)
    (loss * scale).backward()
    return loss.detach(), lr.grad


@functools.lru_cache(maxsize=None)
def reference(shape, dt, eps):
    lg, lab, weight = case(shape, dt)
    return torch_loss(lg, lab, weight, eps, 3.0)


def nchw(dl, shape):
    B, h, w, _, _, ncls = shape
    return dl.view(B, h, w, ncls).permute(0, 3, 1, 2)


def close_loss(out, ref):
    got = (out[0] / out[1].clamp_min(1.0)).item()
    return abs(got - ref.item()) <= LOSS_RTOL * abs(ref.item())


# ---------------------------------------------------------------- 1. weights + smoothing vs torch
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_weighted_smoothed_loss_and_gradient(shape, dt, eps):
    """Both the two-call path (fwd, bwd) and, at factors 4 / 8, the one-pass loss + gradient partials with a
    loss scale of 3, against torch fp32; the count is the valid pixels (a zero-weight class included); a
    second run is bitwise equal."""
    k = K()
    B, h, w, H, W, ncls = shape
    lg, lab, weight = case(shape, dt)
    rows = lg.view(-1, ncls)
    ref_loss, ref_grad = reference(shape, dt, eps)
    gs = torch.full((1,), 3.0, device=DEV)
    out = k.seg_loss_opts_fwd(rows, B, h, w, ncls, lab, weight, eps)
    dl = k.seg_loss_opts_bwd(rows, B, h, w, ncls, lab, out, weight, eps, gscale=gs)
    print(f"two-call {shape} {dt} eps={eps}: loss {(out[0] / out[1]).item():.6f} vs {ref_loss.item():.6f}, "
          f"grad rel {rel(nchw(dl, shape), ref_grad):.2e}")
    assert out[1].item() == (lab != IGNORE).sum().item()
    assert close_loss(out, ref_loss)
    assert rel(nchw(dl, shape), ref_grad) < GRAD_TOL
    out2 = k.seg_loss_opts_fwd(rows, B, h, w, ncls, lab, weight, eps)
    dl2 = k.seg_loss_opts_bwd(rows, B, h, w, ncls, lab, out2, weight, eps, gscale=gs)
    assert torch.equal(out, out2) and torch.equal(dl, dl2)
    if not k.seg_loss_grad_partials_size(B, h, w, ncls, H, W):  # S = 2 and the non-integer factor
        return
    fout, part = k.seg_loss_opts_fwd_grad(rows, B, h, w, ncls, lab, weight, eps)
    fdl = k.seg_loss_bwd_gather(part, B, h, w, ncls, fout, gs, torch.float32)
    fdl16 = k.seg_loss_bwd_gather(part, B, h, w, ncls, fout, gs, dt)
    print(f"fused    {shape} {dt} eps={eps}: loss {(fout[0] / fout[1]).item():.6f}, grad rel "
          f"{rel(nchw(fdl, shape), ref_grad):.2e}, in {dt} {rel(nchw(fdl16.float(), shape), ref_grad):.2e}")
    assert fout[1].item() == out[1].item() and close_loss(fout, ref_loss)
    assert rel(nchw(fdl, shape), ref_grad) < GRAD_TOL
    assert rel(nchw(fdl16.float(), shape), ref_grad) < (GRAD_TOL if dt == torch.float32 else GRAD_TOL16)
    fout2, part2 = k.seg_loss_opts_fwd_grad(rows, B, h, w, ncls, lab, weight, eps)
    assert torch.equal(fout, fout2) and torch.equal(fdl, k.seg_loss_bwd_gather(part2, B, h, w, ncls, fout2, gs,
                                                                              torch.float32))


# ---------------------------------------------------------------- 2. neutral options = the plain kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_neutral_options_equal_the_plain_entry_points(shape, dt):
    """weight = ones (or None), eps = 0: loss and gradient torch.equal to dfm_seg_loss_fwd / bwd / fwd_grad."""
    k = K()
    B, h, w, H, W, ncls = shape
    lg, lab, _ = case(shape, dt)
    rows = lg.view(-1, ncls)
    gs = torch.full((1,), 3.0, device=DEV)
    out = k.seg_loss_fwd(rows, B, h, w, ncls, lab)
    dl = k.seg_loss_bwd(rows, B, h, w, ncls, lab, out, gscale=gs)
    for weight in (torch.ones(ncls, device=DEV), None):
        o = k.seg_loss_opts_fwd(rows, B, h, w, ncls, lab, weight, 0.0)
        assert torch.equal(o, out)
        assert torch.equal(k.seg_loss_opts_bwd(rows, B, h, w, ncls, lab, o, weight, 0.0, gscale=gs), dl)
        if k.seg_loss_grad_partials_size(B, h, w, ncls, H, W):
            fo, fp = k.seg_loss_fwd_grad(rows, B, h, w, ncls, lab)
            go, gp = k.seg_loss_opts_fwd_grad(rows, B, h, w, ncls, lab, weight, 0.0)
            assert torch.equal(fo, go)
            assert torch.equal(k.seg_loss_bwd_gather(fp, B, h, w, ncls, fo, gs, dt),
                               k.seg_loss_bwd_gather(gp, B, h, w, ncls, go, gs, dt))


# ---------------------------------------------------------------- 3. hard example mining
def oracle_prob(lg, lab):
    """softmax probability of the true class of the upsampled logits, float64 (0-filled where ignored)."""
    H, W = lab.shape[-2:]
    up = F.interpolate(lg.double().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=False)
    valid = lab != IGNORE
    return F.softmax(up, dim=1).gather(1, (lab * valid).unsqueeze(1)).squeeze(1), valid


def mined_loss_and_grad(shape, lg, lab, weight, eps, thresh, k_kept):
    """SegLossFn with every option on: (loss, d(3 loss)/d logits rows in the logits dtype)."""
    from dformer_amd.decoders import SegLossFn
    B, h, w, _, _, ncls = shape
    rows = lg.view(-1, ncls).clone().requires_grad_()
    loss = SegLossFn.apply(rows, B, h, w, lab, IGNORE, weight, eps, thresh, k_kept)
    (loss * 3.0).backward()
    return loss.detach(), rows.grad


@pytest.mark.parametrize("regime", ["kth_above_thresh", "thresh_above_kth"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", OHEM_SHAPES)
def test_ohem_selection(shape, dt, regime):
    """The device-side k-th smallest probability, threshold = max(thresh, k-th) and the rewritten labels
    against a float64 sort, in both regimes; then loss and gradient on the kernel's own labels.
    The labels are compared outside the band |p - threshold| <= 1e-4, which may hold at most 2 % of the valid
    pixels (fp32 probabilities deviate from fp64 by <= 5e-7 on these cases and the band holds <= 0.54 %; the
    8 x 12 plane's 177 pixels would reach 1.1 % and are left out of OHEM_SHAPES)."""
    k = K()
    B, h, w, H, W, ncls = shape
    lg, lab, weight = case(shape, dt)
    rows = lg.view(-1, ncls)
    p, valid = oracle_prob(lg, lab)
    n = int(valid.sum())
    assert n >= 800
    # a floor of 0.001 lies under the 3n/4-th smallest probability for every class count here (the 64-class
    # cases have it near 0.009), 0.6 above the n/8-th smallest even with 2 classes
    thresh, kk = (0.001, 3 * n // 4) if regime == "kth_above_thresh" else (0.6, n // 8)
    kth = p[valid].sort().values[kk - 1].item()
    assert (kth > thresh) == (regime == "kth_above_thresh"), (kth, thresh)  # the regime this case is meant for
    ref_thr = max(thresh, kth)
    new_lab, prob, stats = k.seg_loss_ohem_relabel(rows, B, h, w, ncls, lab, thresh, kk)
    perr = (prob.double() - p)[valid].abs().max().item()
    band = valid & ((p - ref_thr).abs() <= 1e-4)
    print(f"ohem {shape} {dt} {regime}: threshold {stats[0].item():.7f} vs {ref_thr:.7f}, prob err {perr:.1e}, "
          f"band {int(band.sum())}/{n}, kept {int((new_lab != IGNORE).sum())}")
    assert stats[1].item() == n
    assert abs(stats[0].item() - ref_thr) <= 1e-5
    assert torch.all(prob[~valid] == 2.0)
    assert int(band.sum()) <= 0.02 * n
    ref_lab = torch.where(valid & (p <= ref_thr), lab, torch.full_like(lab, IGNORE))
    assert torch.equal(new_lab[~band], ref_lab[~band])
    assert torch.all((new_lab == lab) | (new_lab == IGNORE))
    if regime == "kth_above_thresh":  # ties kept: at least k pixels survive
        assert int((new_lab != IGNORE).sum()) >= kk
    # loss and gradient of the whole criterion given the kernel's own selection
    loss, grad = mined_loss_and_grad(shape, lg, lab, weight, 0.1, thresh, kk)
    ref_loss, ref_grad = torch_loss(lg, new_lab, weight, 0.1, 3.0)
    gerr = rel(nchw(grad.float(), shape), ref_grad)
    print(f"     loss {loss.item():.6f} vs {ref_loss.item():.6f}, grad rel {gerr:.2e}")
    assert abs(loss.item() - ref_loss.item()) <= LOSS_RTOL * abs(ref_loss.item())
    assert gerr < (GRAD_TOL if dt == torch.float32 else GRAD_TOL16)
    again = k.seg_loss_ohem_relabel(rows, B, h, w, ncls, lab, thresh, kk)
    assert torch.equal(again[0], new_lab) and torch.equal(again[1], prob) and torch.equal(again[2], stats)
    loss2, grad2 = mined_loss_and_grad(shape, lg, lab, weight, 0.1, thresh, kk)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", OHEM_SHAPES)
def test_ohem_keeps_everything_when_nothing_is_mined(shape, dt):
    """min_kept > num_valid and min_kept == 0 (loss_opr.py:167,174) keep every valid pixel; an all-ignored
    plane gives loss 0 and a zero gradient."""
    k = K()
    B, h, w, H, W, ncls = shape
    lg, lab, weight = case(shape, dt)
    rows = lg.view(-1, ncls)
    n = int((lab != IGNORE).sum())
    plain_loss, plain_grad = mined_loss_and_grad(shape, lg, lab, weight, 0.1, None, 0)
    for kk in (n + 1, 0):
        new_lab, _, stats = k.seg_loss_ohem_relabel(rows, B, h, w, ncls, lab, 0.3, kk)
        assert torch.equal(new_lab, lab) and stats[1].item() == n and stats[0].item() == 1.0
        loss, grad = mined_loss_and_grad(shape, lg, lab, weight, 0.1, 0.3, kk)
        assert torch.equal(loss, plain_loss) and torch.equal(grad, plain_grad)
    new_lab, _, stats = k.seg_loss_ohem_relabel(rows, B, h, w, ncls, lab, 0.3, n)  # k = num_valid still mines
    assert stats[0].item() < 1.0 or int((new_lab != IGNORE).sum()) == n
    none = torch.full_like(lab, IGNORE)
    for kk in (0, 5, n):
        new_lab, _, stats = k.seg_loss_ohem_relabel(rows, B, h, w, ncls, none, 0.3, kk)
        assert torch.equal(new_lab, none) and stats[1].item() == 0
        loss, grad = mined_loss_and_grad(shape, lg, none, weight, 0.1, 0.3, kk)
        assert loss.item() == 0.0 and torch.all(grad == 0)


# ---------------------------------------------------------------- 4. EncoderDecoder + FusedSegLoss
class Cfg(dict):
    __getattr__ = dict.__getitem__


def module_oracle(low, lab, crit):
    """The criterion's definition on the head's logits `low` [B, C, h, w]: float64 selection, fp32 loss.
    -> (loss, d loss / d low)."""
    H, W = lab.shape[-2:]
    lr = low.detach().float().requires_grad_()
    up = F.interpolate(lr, (H, W), mode="bilinear", align_corners=False)
    valid = lab != IGNORE
    kept, n = valid, int(valid.sum())
    if crit.ohem_thresh is not None and 0 < crit.ohem_min_kept <= n:
        p = F.softmax(up.detach().double(), dim=1).gather(1, (lab * valid).unsqueeze(1)).squeeze(1)
        kth = p[valid].sort().values[crit.ohem_min_kept - 1].item()
        kept = valid & (p <= max(crit.ohem_thresh, kth))
    tgt = torch.where(kept, lab, torch.full_like(lab, IGNORE))
    ce = F.cross_entropy(up, tgt, weight=crit.weight, reduction="none", ignore_index=IGNORE,
                         label_smoothing=crit.label_smoothing)
    loss = ce.sum() / kept.sum().clamp_min(1)
    loss.backward()
    return loss.detach(), lr.grad


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("aux_rate", [0, 0.4])
def test_encoder_decoder_with_fused_seg_loss(aux_rate, dt):
    """DFormer-Tiny + ham (and with the aux head, aux_rate = 0.4) at 2 x 64 x 96 with FusedSegLoss(weight,
    0.1, ohem_thresh=0.7, ohem_min_kept=n/4): the loss and the gradient reaching the low-res logits of each
    head against the torch oracle built from those logits (the aux head mined on its own probabilities)."""
    from dformer_amd.losses import FusedSegLoss
    from dformer_amd.segmentor import EncoderDecoder
    import bench
    cfg = Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=40, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=IGNORE, aux_rate=aux_rate)
    torch.manual_seed(3)
    weight = 0.5 + 1.5 * torch.rand(40)
    weight[20] = 0.0
    rgb, dep, lab = bench.synthetic_batch(2, 64, 96, 40, torch.device(DEV, 0), 5)
    crit = FusedSegLoss(IGNORE, weight, 0.1, ohem_thresh=0.7, ohem_min_kept=int((lab != IGNORE).sum()) // 4)
    model = EncoderDecoder(cfg=cfg, criterion=crit)
    model.decode_head.dropout_ratio = 0.0
    model = model.to(DEV).train()
    if dt != torch.float32:
        model.set_compute_dtype(dt)
    model.return_logits = False
    heads = {}
    if aux_rate:
        def keep(_m, _i, out):
            out.retain_grad()
            heads["aux"] = out
        model.aux_head.register_forward_hook(keep)
    loss, low = model(rgb, dep, lab)
    low.retain_grad()
    loss.backward()
    ref, gref = module_oracle(low, lab, crit)
    tol = GRAD_TOL if low.dtype == torch.float32 else GRAD_TOL16
    print(f"module aux_rate={aux_rate} {dt}: low {low.dtype}, main grad rel {rel(low.grad.float(), gref):.2e}")
    assert rel(low.grad.float(), gref) < tol
    if aux_rate:
        aref, agref = module_oracle(heads["aux"], lab, crit)
        ref = ref + aux_rate * aref
        assert rel(heads["aux"].grad.float(), aux_rate * agref) < tol
    print(f"       loss {loss.item():.6f} vs {ref.item():.6f}")
    assert abs(loss.item() - ref.item()) <= LOSS_RTOL * abs(ref.item())


def test_graphed_train_step_replays_the_criterion():
    """A step with weights, smoothing and active mining captures into a HIP graph (the threshold is found on
    the device) and its replays give the eager steps' losses bit for bit."""
    import bench
    from dformer_amd.losses import FusedSegLoss
    from dformer_amd.segmentor import EncoderDecoder
    from dformer_amd.train import FusedAdamW, GraphedTrainStep, train_step
    dev = torch.device(DEV, 0)
    rgb, dep, lab = bench.synthetic_batch(2, 64, 96, 40, dev, 5)

    def make():
        cfg = bench.make_cfg("DFormer-Tiny", "ham")
        cfg["drop_path_rate"] = 0.0
        torch.manual_seed(3)
        weight = 0.5 + 1.5 * torch.rand(40)
        crit = FusedSegLoss(IGNORE, weight, 0.1, ohem_thresh=0.02, ohem_min_kept=2000)
        m = EncoderDecoder(cfg=cfg, criterion=crit)
        m.decode_head.dropout_ratio = 0.0
        m = m.to(dev).set_compute_dtype(torch.bfloat16)
        m.return_logits = False
        return cfg, m.train()

    (cfg, ma), (_, mb) = make(), make()
    gb = torch.Generator(device=dev)
    gb.manual_seed(11)
    bases = torch.rand(2, 512, 64, device=dev, generator=gb)
    bases = bases / bases.norm(dim=1, keepdim=True)
    for m in (ma, mb):
        m.decode_head.hamburger.ham.injected_bases = bases
    oa = FusedAdamW(ma, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
    ob = FusedAdamW(mb, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
    la = [train_step(ma, oa, rgb, dep, lab).item() for _ in range(4)]
    g = GraphedTrainStep(mb, ob, rgb, dep, lab, warmup=2)
    lb = [g().item() for _ in range(2)]
    assert all(x == x and abs(x) != float("inf") for x in la) and la[2:] == lb, (la, lb)
    for ga, gb_ in zip(oa.groups, ob.groups):
        assert torch.equal(ga.flat, gb_.flat)
