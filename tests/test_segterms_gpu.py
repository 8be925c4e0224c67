"""The focal and Tversky / Dice terms of the fused segmentation loss on the GPU (csrc/criterion/seg_terms.hip:
dfc_seg_terms_fwd / _bwd; criterion.SegTermsFn; losses.FusedSegLoss in EncoderDecoder). Every oracle is torch
float64 autograd on F.interpolate of the stored logits, written here from torch primitives."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# (B, h, w, H, W, ncls): the smallest that reach each geometry (interior and edge cells, a partial block, more
# than one image so per-image sums cannot mix) and both block sizes of the kernels (ncls <= 56, above)
SHAPES = [(2, 5, 7, 40, 56, 40),   # factor 8
          (2, 6, 5, 24, 20, 37),   # factor 4, odd class count
          (2, 7, 9, 28, 36, 64),   # factor 4, 128-thread blocks
          (2, 4, 6, 8, 12, 64),    # factor 2, one partial block per image
          (1, 7, 9, 30, 41, 19),   # non-integer factor
          (2, 5, 7, 40, 56, 2),    # the Trav head
          (3, 3, 4, 12, 16, 5)]    # three images
IGNORE = 255
# tolerances of this kernel family (test_segloss_opts_gpu.py)
LOSS_RTOL, GRAD_TOL, GRAD_TOL16 = 1e-4, 1e-3, 4e-3
SCALE = 3.0  # the loss scale passed through gscale
# (name, focal_gamma, has_pixel, region (alpha, beta, smooth) or None, region_weight)
TERMS = [("focal2", 2.0, True, None, 1.0), ("focal0.5", 0.5, True, None, 1.0),
         ("tversky", 0.0, False, (0.3, 0.7, 1.0), 1.0), ("dice", 0.0, False, (0.5, 0.5, 1.0), 1.0),
         ("both", 2.0, True, (0.3, 0.7, 1.0), 0.7)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def C():
    from dformer_amd import criterion
    return criterion


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def case(shape, dt):
    """(logits [B, h, w, ncls] in dt, labels with 10 % ignored and class C - 1 absent from the last image, weights
    U(0.5, 2) with one class at 0), generated on the CPU; shared by the tests, never modified."""
    B, h, w, H, W, ncls = shape
    g = torch.Generator().manual_seed(1000 * h + ncls)
    lg = (3 * torch.randn(B, h, w, ncls, generator=g)).to(dt)
    lab = torch.randint(0, ncls, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = IGNORE
    lab[-1][lab[-1] == ncls - 1] = 0
    weight = 0.5 + 1.5 * torch.rand(ncls, generator=g)
    weight[ncls // 2] = 0.0
    return lg.to(DEV), lab.to(DEV), weight.to(DEV)


def definition(up, lab, weight, gamma, has_pixel, region, rw):
    """The two terms on full-resolution logits `up` [B, C, H, W] (any float dtype) -> (loss, L_pix sum, L_reg)."""
    ncls = up.shape[1]
    w = torch.ones(ncls, dtype=up.dtype, device=up.device) if weight is None else weight.to(up.dtype)
    valid = lab != IGNORE
    safe = (lab * valid).unsqueeze(1)
    logp = F.log_softmax(up, dim=1)
    p = logp.exp()
    loss, pix, reg = up.new_zeros(()), up.new_zeros(()), up.new_zeros(())
    if has_pixel:
        logq = logp.gather(1, safe).squeeze(1)
        onehot = torch.zeros_like(p).scatter_(1, safe, 1.0)
        # 1 - q as the sum of the others; the clamp keeps the derivative of x^gamma finite where x underflows to 0
        omq = (p * (1.0 - onehot)).sum(1).clamp_min(torch.finfo(up.dtype).tiny)
        focal = omq.pow(gamma) if gamma > 0 else torch.ones_like(omq)
        pix = (w[safe.squeeze(1)] * focal * -logq * valid).sum()
        loss = pix / valid.sum().clamp_min(1)
    if region is not None:
        alpha, beta, smooth = region
        v = valid.unsqueeze(1).to(up.dtype)
        onehot = torch.zeros_like(p).scatter_(1, safe, 1.0) * v
        TP, SP, SY = (p * onehot).sum((2, 3)), (p * v).sum((2, 3)), onehot.sum((2, 3))
        T = (TP + smooth) / (TP + alpha * (SP - TP) + beta * (SY - TP) + smooth)
        reg = ((w * (1.0 - T)).sum(1) / ncls).mean()
        loss = loss + rw * reg
    return loss, pix, reg


def oracle(lg, lab, weight, gamma, has_pixel, region, rw, scale=SCALE):
    """float64 autograd on F.interpolate of the stored logits -> (loss, pixel sum, L_reg, scale * d loss / d
    logits as NCHW)."""
    H, W = lab.shape[-2:]
    lr = lg.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    up = F.interpolate(lr, (H, W), mode="bilinear", align_corners=False)
    loss, pix, reg = definition(up, lab, weight, gamma, has_pixel, region, rw)
    (loss * scale).backward()
    return loss.detach(), pix.detach(), reg.detach(), lr.grad


@functools.lru_cache(maxsize=None)
def reference(shape, dt, terms):
    lg, lab, weight = case(shape, dt)
    return oracle(lg, lab, weight, *terms[1:])


def nchw(dl, shape):
    B, h, w, _, _, ncls = shape
    return dl.view(B, h, w, ncls).permute(0, 3, 1, 2)


def run(shape, lg, lab, weight, terms, scale=SCALE):
    """The two C entry points -> (stats, out, dlogits rows in the logits' dtype, loss)."""
    c = C()
    B, h, w, _, _, ncls = shape
    _, gamma, has_pixel, region, rw = terms
    rows = lg.view(-1, ncls)
    desc = c.make_desc(gamma, has_pixel, region)
    gs = torch.full((1,), scale, device=DEV)
    stats, out = c.seg_terms_fwd(rows, B, h, w, lab, desc, weight)
    dl = c.seg_terms_bwd(rows, B, h, w, lab, desc, stats, out, gs, rw, weight)
    loss = (out[0] / out[1].clamp_min(1.0) if has_pixel else 0.0) + (rw * out[2] if region is not None else 0.0)
    return stats, out, dl, loss


def grad_tol(dt):
    return GRAD_TOL if dt == torch.float32 else GRAD_TOL16


# ---------------------------------------------------------------- 1. each term against float64
@pytest.mark.parametrize("terms", TERMS, ids=[t[0] for t in TERMS])
@pytest.mark.parametrize("dt", DTYPES, ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_terms_against_float64(shape, dt, terms):
    """Focal alone, region alone and both (the region gradient is several times smaller than the focal one and
    would hide under a max-norm over the sum): loss, exact valid count, gradient with a loss scale of 3 through
    gscale, and a second run bitwise equal."""
    lg, lab, weight = case(shape, dt)
    ref_loss, ref_pix, ref_reg, ref_grad = reference(shape, dt, terms)
    stats, out, dl, loss = run(shape, lg, lab, weight, terms)
    gerr = rel(nchw(dl.float(), shape), ref_grad)
    print(f"{terms[0]} {shape} {dt}: loss {float(loss):.7f} vs {ref_loss.item():.7f}, pixel sum {out[0].item():.6f} vs "
          f"{ref_pix.item():.6f}, L_reg {out[2].item():.7f} vs {ref_reg.item():.7f}, grad rel {gerr:.2e}")
    assert dl.dtype == dt and tuple(dl.shape) == (shape[0] * shape[1] * shape[2], shape[5])
    assert out[1].item() == (lab != IGNORE).sum().item()
    assert abs(float(loss) - ref_loss.item()) <= LOSS_RTOL * abs(ref_loss.item())
    if terms[2]:
        assert abs(out[0].item() - ref_pix.item()) <= LOSS_RTOL * abs(ref_pix.item())
    else:
        assert out[0].item() == 0.0
    if terms[3] is not None:
        assert abs(out[2].item() - ref_reg.item()) <= LOSS_RTOL * abs(ref_reg.item())
    else:
        assert out[2].item() == 0.0 and torch.all(stats == 0)
    assert gerr < grad_tol(dt)
    stats2, out2, dl2, _ = run(shape, lg, lab, weight, terms)
    assert torch.equal(stats, stats2) and torch.equal(out, out2) and torch.equal(dl, dl2)


def test_unweighted_terms():
    """weight = NULL is weight = 1."""
    shape, dt, terms = SHAPES[0], torch.float32, TERMS[4]
    lg, lab, _ = case(shape, dt)
    ref_loss, _, _, ref_grad = oracle(lg, lab, None, *terms[1:])
    _, _, dl, loss = run(shape, lg, lab, None, terms)
    _, _, dl1, loss1 = run(shape, lg, lab, torch.ones(shape[5], device=DEV), terms)
    assert abs(float(loss) - ref_loss.item()) <= LOSS_RTOL * abs(ref_loss.item())
    assert rel(nchw(dl, shape), ref_grad) < GRAD_TOL
    assert torch.equal(dl, dl1) and float(loss) == float(loss1)


# ---------------------------------------------------------------- 2. stats
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_stats(shape):
    """SY is the per-image, per-class label histogram exactly; TP <= SP; SP summed over the classes is the
    per-image valid count (the probabilities of a pixel sum to 1)."""
    B, ncls = shape[0], shape[5]
    lg, lab, weight = case(shape, torch.float32)
    stats, out, _, _ = run(shape, lg, lab, weight, TERMS[2])
    hist = torch.stack([torch.bincount(lab[b][lab[b] != IGNORE], minlength=ncls) for b in range(B)])
    assert torch.equal(stats[..., 2], hist.float())
    assert hist[-1, ncls - 1] == 0 and stats[-1, ncls - 1, 0] == 0  # the absent class
    assert torch.all(stats[..., 0] <= stats[..., 1])
    count = (lab != IGNORE).flatten(1).sum(1).double()
    assert ((stats[..., 1].double().sum(1) - count).abs() <= 1e-5 * count).all()
    H, W = lab.shape[-2:]
    up = F.interpolate(lg.double().permute(0, 3, 1, 2), (H, W), mode="bilinear", align_corners=False)
    pv = F.softmax(up, 1) * (lab != IGNORE).unsqueeze(1)
    onehot = torch.zeros_like(pv).scatter_(1, (lab * (lab != IGNORE)).unsqueeze(1), 1.0)
    assert rel(stats[..., 1], pv.sum((2, 3))) < LOSS_RTOL and rel(stats[..., 0], (pv * onehot).sum((2, 3))) < LOSS_RTOL


# ---------------------------------------------------------------- 3. gamma = 0 ties the two libraries' tap rules
@pytest.mark.parametrize("dt", DTYPES, ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_gamma_zero_is_the_weighted_cross_entropy_of_the_model_library(shape, dt):
    from dformer_amd import kernels as K
    B, h, w, H, W, ncls = shape
    lg, lab, weight = case(shape, dt)
    rows = lg.view(-1, ncls)
    gs = torch.full((1,), SCALE, device=DEV)
    kout = K.seg_loss_opts_fwd(rows, B, h, w, ncls, lab, weight, 0.0)
    kdl = K.seg_loss_opts_bwd(rows, B, h, w, ncls, lab, kout, weight, 0.0, gscale=gs)
    _, out, dl, _ = run(shape, lg, lab, weight, ("ce", 0.0, True, None, 1.0))
    print(f"gamma=0 {shape} {dt}: sum {out[0].item():.6f} vs {kout[0].item():.6f}, grad rel "
          f"{rel(dl.float(), kdl):.2e}")
    assert out[1].item() == kout[1].item()
    assert abs(out[0].item() - kout[0].item()) <= LOSS_RTOL * abs(kout[0].item())
    assert rel(dl.float(), kdl) < grad_tol(dt)


# ---------------------------------------------------------------- 4. saturation
@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["float32x30", "float16_6e4"])
def test_saturated_logits(dt, gamma):
    """fp32 logits scaled x30 (probabilities of exactly 0 and 1 in float32); fp16 logits with +-6e4 entries: one
    class at +6e4 and one at -6e4 over the top two cell rows of image 0. Loss and gradient stay finite and agree
    with float64, absolutely to 1e-6 where the float64 gradient is itself below 1e-3."""
    shape = SHAPES[0]
    B, h, w, H, W, ncls = shape
    lg, lab, weight = case(shape, dt)
    if dt == torch.float32:
        lg = lg * 30.0
    else:
        lg = lg.clone()
        lg[0, :2, :, 3] = 6e4
        lg[0, :2, :, 7] = -6e4
    for terms in (("focal", gamma, True, None, 1.0), ("both", gamma, True, (0.3, 0.7, 1.0), 1.0)):
        ref_loss, _, _, ref_grad = oracle(lg, lab, weight, *terms[1:])
        _, out, dl, loss = run(shape, lg, lab, weight, terms)
        got = nchw(dl.float(), shape).double()
        print(f"saturated {dt} gamma={gamma} {terms[0]}: loss {float(loss):.6f} vs {ref_loss.item():.6f}, grad max "
              f"{ref_grad.abs().max().item():.3e}, abs err {(got - ref_grad).abs().max().item():.2e}")
        assert torch.isfinite(out).all() and torch.isfinite(dl).all()
        assert abs(float(loss) - ref_loss.item()) <= LOSS_RTOL * abs(ref_loss.item())
        if ref_grad.abs().max().item() < 1e-3:
            assert (got - ref_grad).abs().max().item() <= 1e-6
        else:
            assert rel(got, ref_grad) < grad_tol(dt)


# ---------------------------------------------------------------- 5. nothing valid
@pytest.mark.parametrize("dt", DTYPES, ids=["float32", "bfloat16", "float16"])
def test_all_labels_ignored(dt):
    shape = SHAPES[1]
    lg, lab, weight = case(shape, dt)
    none = torch.full_like(lab, IGNORE)
    for terms in TERMS:
        stats, out, dl, loss = run(shape, lg, none, weight, terms)
        assert float(loss) == 0.0 and out[1].item() == 0.0 and torch.all(dl == 0) and torch.all(stats == 0)


# ---------------------------------------------------------------- 6. no full-resolution tensor
def test_no_full_resolution_tensor():
    """Forward + backward of SegTermsFn at the first shape in fp32 allocate less than a quarter of the
    full-resolution logits, B C H W 4 bytes (by shapes the block partials are about 1/128 of them)."""
    from dformer_amd.criterion import SegTermsFn
    shape = SHAPES[0]
    B, h, w, H, W, ncls = shape
    lg, lab, weight = case(shape, torch.float32)
    rows = lg.view(-1, ncls).clone().requires_grad_()
    SegTermsFn.apply(rows, B, h, w, lab, IGNORE, weight, 2.0, True, (0.3, 0.7, 1.0), 1.0).backward()  # warm-up
    rows.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    loss = SegTermsFn.apply(rows, B, h, w, lab, IGNORE, weight, 2.0, True, (0.3, 0.7, 1.0), 1.0)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    full = B * ncls * H * W * 4
    print(f"peak rise {rise} bytes, full-resolution logits {full} bytes")
    assert torch.isfinite(loss) and rows.grad is not None
    assert rise < full // 4


# ---------------------------------------------------------------- 7. EncoderDecoder end to end
class Cfg(dict):
    __getattr__ = dict.__getitem__


def tiny_model(crit, num_classes=40, aux_rate=0):
    """DFormer-Tiny + ham with the weights, inputs and NMF bases of __graft_entry__.smoke()."""
    import numpy as np
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import gen
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=num_classes,
              drop_path_rate=0.0, bn_eps=1e-3, bn_momentum=0.1, background=IGNORE, aux_rate=aux_rate)
    model = EncoderDecoder(cfg=cfg, criterion=crit)
    model.decode_head.dropout_ratio = 0.0
    sd = model.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    state = {k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()}
    model.load_state_dict(state)
    model = model.cuda().train()
    B, H, W = 2, 64, 96
    bases = torch.from_numpy(gen.nmf_bases(B, 512, 64)).float()
    model.decode_head.hamburger.ham.injected_bases = bases
    rgb_np, dep_np = gen.rgb_depth(B, H, W)
    lab = torch.from_numpy(gen.labels(B, H, W))
    model.return_logits = False
    return model, state, bases, torch.from_numpy(rgb_np).float(), torch.from_numpy(dep_np).float(), lab


def class_weights(n):
    torch.manual_seed(3)
    weight = 0.5 + 1.5 * torch.rand(n)
    weight[n // 2] = 0.0
    return weight


@pytest.mark.parametrize("num_classes", [40, 2])
def test_encoder_decoder_end_to_end(num_classes):
    """FusedSegLoss(focal_gamma=2, region='tversky', weight) in the segmentor against the float64 oracle model:
    its low-res logits, the definition applied to their upsample, backpropagated (smoke()'s bounds). With 2
    classes (the Trav head's width) the labels are taken modulo 2, ignored pixels kept."""
    import dformer_ref as R  # noqa: F401  (tiny_model puts oracle/ on the path)
    from dformer_amd.losses import FusedSegLoss
    weight = class_weights(num_classes)
    crit = FusedSegLoss(IGNORE, weight, focal_gamma=2.0, region="tversky")
    model, state, bases, rgb, dep, lab = tiny_model(crit, num_classes)
    if num_classes == 2:
        lab = torch.where(lab == IGNORE, lab, lab % 2)
    loss, low = model(rgb.cuda(), dep.cuda(), lab.cuda())
    loss.backward()
    torch.cuda.synchronize()
    p = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in state.items()
         if not k.endswith("num_batches_tracked")}
    bufs = {k: v.clone() for k, v in p.items() if "running" in k}
    _, ref_low = R.segmentor_forward(p, "DFormer-Tiny", "ham", rgb.double(), dep.double(), bases.double(), True,
                                     buffers=bufs)
    up = F.interpolate(ref_low, lab.shape[-2:], mode="bilinear", align_corners=False)
    ref_loss, _, _ = definition(up, lab, weight, 2.0, True, (0.3, 0.7, 1.0), 1.0)
    ref_loss.backward()
    name = "encoder_backbone.stages.1.0.attn.q.weight"
    gw = dict(model.named_parameters())[name].grad.double().cpu()
    gerr = rel(gw, p[name].grad)
    print(f"end to end C={num_classes}: loss {loss.item():.6f} vs {ref_loss.item():.6f}, grad rel {gerr:.2e}")
    assert abs(loss.item() - ref_loss.item()) < 1e-3 * abs(ref_loss.item())
    assert gerr < 1e-2


def test_encoder_decoder_applies_the_criterion_to_the_aux_head():
    """aux_rate = 0.4: loss = def(main) + 0.4 def(aux) on each head's own logits, and the gradient reaching each
    head's low-res logits is the definition's (the oracle model has no aux head, so the heads' logits are taken
    from the model and the definition is evaluated on them in float64)."""
    from dformer_amd.losses import FusedSegLoss
    weight = class_weights(40)
    crit = FusedSegLoss(IGNORE, weight, focal_gamma=2.0, region="tversky")
    model, _, _, rgb, dep, lab = tiny_model(crit, 40, aux_rate=0.4)
    heads = {}

    def keep(_m, _i, out):
        out.retain_grad()
        heads["aux"] = out
    model.aux_head.register_forward_hook(keep)
    lab = lab.cuda()
    loss, low = model(rgb.cuda(), dep.cuda(), lab)
    low.retain_grad()
    loss.backward()
    total = 0.0
    for t, rate in ((low, 1.0), (heads["aux"], 0.4)):
        lr = t.detach().double().requires_grad_()
        up = F.interpolate(lr, lab.shape[-2:], mode="bilinear", align_corners=False)
        ref, _, _ = definition(up, lab, weight.to(DEV), 2.0, True, (0.3, 0.7, 1.0), 1.0)
        ref.backward()
        total += rate * ref.item()
        assert rel(t.grad.float(), rate * lr.grad) < GRAD_TOL
    print(f"aux: loss {loss.item():.6f} vs {total:.6f}")
    assert abs(loss.item() - total) <= LOSS_RTOL * abs(total)


def test_region_only_keeps_the_pixel_term_on_segloss():
    """region alone with smoothing and mining: SegLossFn's loss (weights, smoothing, mining) + region_weight *
    L_reg on the original labels, loss and gradient."""
    from dformer_amd.decoders import SegLossFn
    from dformer_amd.losses import FusedSegLoss
    weight = class_weights(40)
    crit = FusedSegLoss(IGNORE, weight, 0.1, ohem_thresh=0.7, ohem_min_kept=1500, region="dice", region_weight=0.5)
    model, _, _, rgb, dep, lab = tiny_model(crit, 40)
    lab = lab.cuda()
    loss, low = model(rgb.cuda(), dep.cuda(), lab)
    low.retain_grad()
    loss.backward()
    B, _, h, w = low.shape
    rows = low.detach().permute(0, 2, 3, 1).reshape(-1, 40).contiguous().requires_grad_()
    pix = SegLossFn.apply(rows, B, h, w, lab, IGNORE, *crit.kernel_options(rows.device))
    pix.backward()
    lr = low.detach().double().requires_grad_()
    up = F.interpolate(lr, lab.shape[-2:], mode="bilinear", align_corners=False)
    _, _, reg = definition(up, lab, weight.to(DEV), 0.0, False, (0.5, 0.5, 1.0), 1.0)
    (0.5 * reg).backward()
    want = nchw(rows.grad, (B, h, w, 0, 0, 40)).double() + lr.grad
    assert abs(loss.item() - (pix.item() + 0.5 * reg.item())) <= LOSS_RTOL * abs(loss.item())
    assert rel(low.grad, want) < GRAD_TOL


# ---------------------------------------------------------------- 8. the default criterion is untouched
DEFAULT_SCRIPT = r"""
import json, os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import torch, torch.nn as nn
import bench
import kernel_variants as kv
from dformer_amd.losses import FusedSegLoss
from dformer_amd.segmentor import EncoderDecoder
dev = torch.device("cuda", 0)
rgb, dep, lab = bench.synthetic_batch(2, 64, 96, 40, dev, 5)
def step(crit):
    cfg = bench.make_cfg("DFormer-Tiny", "ham")
    cfg["drop_path_rate"] = 0.0
    torch.manual_seed(3)
    m = EncoderDecoder(cfg=cfg, criterion=crit).to(dev).train()
    m.decode_head.dropout_ratio = 0.0
    m.return_logits = False
    gb = torch.Generator(device=dev)
    gb.manual_seed(11)
    bases = torch.rand(2, 512, 64, device=dev, generator=gb)
    m.decode_head.hamburger.ham.injected_bases = bases / bases.norm(dim=1, keepdim=True)
    with kv.Trace() as t:
        loss, _ = m(rgb, dep, lab)
        loss.backward()
        torch.cuda.synchronize()
    return t.launched, loss.item()
mapped = lambda: int("libdformer_criterion.so" in open("/proc/self/maps").read())
a = step(nn.CrossEntropyLoss(reduction="none", ignore_index=255))
b = step(FusedSegLoss())
before = [mapped(), int("dformer_amd.criterion" in sys.modules)]
import dformer_amd.criterion
c = step(FusedSegLoss())
print(json.dumps(dict(before=before, after=mapped(), n=len(a[0]), same_ab=a == b, same_ac=a == c,
                      loss_kernels=sorted({k for k in a[0] if "seg_loss" in k}))))
"""


def test_default_criterion_is_unchanged():
    """nn.CrossEntropyLoss and FusedSegLoss(): one training step launches the same kernels in the same order and
    gives the same loss, before and after dformer_amd.criterion is imported, and the library is not mapped
    until then (a fresh process: this one has imported it)."""
    r = subprocess.run([sys.executable, "-c", DEFAULT_SCRIPT % dict(root=ROOT)], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["before"] == [0, 0] and out["after"] == 1
    assert out["n"] > 100 and out["same_ab"] and out["same_ac"]
    assert out["loss_kernels"] and all("seg_terms" not in k for k in out["loss_kernels"])


# ---------------------------------------------------------------- 9. graph capture
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16_loss_scaler"])
def test_graphed_train_step_replays_the_terms(dt):
    """A step with the focal and region terms captures into a HIP graph; three replays give the losses of three
    eager steps bit for bit. In fp16 the LossScaler's scale reaches the kernels through gscale."""
    import bench
    from dformer_amd.losses import FusedSegLoss
    from dformer_amd.segmentor import EncoderDecoder
    from dformer_amd.train import FusedAdamW, GraphedTrainStep, train_step
    dev = torch.device(DEV, 0)
    rgb, dep, lab = bench.synthetic_batch(2, 64, 96, 40, dev, 5)

    def make():
        cfg = bench.make_cfg("DFormer-Tiny", "ham")
        cfg["drop_path_rate"] = 0.0
        crit = FusedSegLoss(IGNORE, class_weights(40), focal_gamma=2.0, region="tversky")
        torch.manual_seed(3)
        m = EncoderDecoder(cfg=cfg, criterion=crit)
        m.decode_head.dropout_ratio = 0.0
        m = m.to(dev).set_compute_dtype(dt)
        m.return_logits = False
        return cfg, m.train()

    (cfg, ma), (_, mb) = make(), make()
    gb = torch.Generator(device=dev)
    gb.manual_seed(11)
    bases = torch.rand(2, 512, 64, device=dev, generator=gb)
    bases = bases / bases.norm(dim=1, keepdim=True)
    for m in (ma, mb):
        m.decode_head.hamburger.ham.injected_bases = bases
    oa = FusedAdamW(ma, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=dt)
    ob = FusedAdamW(mb, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=dt)
    assert (oa.scaler is not None) == (dt == torch.float16)
    la = [train_step(ma, oa, rgb, dep, lab).item() for _ in range(5)]
    g = GraphedTrainStep(mb, ob, rgb, dep, lab, warmup=2)
    lb = [g().item() for _ in range(3)]
    print(la, lb)
    assert all(x == x and abs(x) != float("inf") for x in la) and la[2:] == lb, (la, lb)
    for ga, gb_ in zip(oa.groups, ob.groups):
        assert torch.equal(ga.flat, gb_.flat)


# ---------------------------------------------------------------- 10. episodes
@pytest.mark.parametrize("opts", [dict(focal_gamma=2.0), dict(region="dice")], ids=["focal", "region"])
def test_meta_forward_refuses_the_terms(opts):
    from dformer_amd.losses import FusedSegLoss
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=2, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=IGNORE, alpha=0.5, temperature=1.0)
    model = EncoderDecoder(cfg=cfg, criterion=FusedSegLoss(IGNORE, **opts)).to(DEV).train()
    B, S, H, W = 1, 1, 64, 96
    s_rgb, s_dep = torch.randn(B, S, 3, H, W, device=DEV), torch.randn(B, S, 1, H, W, device=DEV)
    s_mask = torch.randint(0, 2, (B, S, H, W), device=DEV)
    q_rgb, q_dep = torch.randn(B, 3, H, W, device=DEV), torch.randn(B, 1, H, W, device=DEV)
    q_gt = torch.randint(0, 2, (B, H, W), device=DEV)
    with pytest.raises(NotImplementedError, match="focal or region"):
        model.meta_forward(s_rgb, s_dep, s_mask, q_rgb, q_dep, q_gt)
