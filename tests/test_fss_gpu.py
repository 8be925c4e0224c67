"""Few-shot episodes on the GPU (models/builder.py:237-320): the fss kernels against float64 (autograd of
F.interpolate, F.cosine_similarity and F.cross_entropy on the CPU, and the collapsed restatement of
fss_common), meta_forward against the reference's float64 golden (oracle/golden_e2e.py), the eager
episode training step and fss_evaluate.

Tolerances, the rule of tests/test_trav_gpu.py: rel-to-max within max(1e-4, 10 x the reference's own float32
error stored in env/); 1e-4 where there is no env entry (the kernel cases). A quantity stored in bf16 is compared
at 2^-8 of its maximum (one bf16 rounding, 2^-9, with a factor 2) against the float64 value on the same
bf16-rounded inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fss_common as FC
import gen
import trav_common as TC
from goldens import fp_rel_err, load, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16_TOL = 2.0 ** -8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.manual_seed(0)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def tol_of(dtype):
    return BF16_TOL if dtype == torch.bfloat16 else 1e-4


def strided(t, pad=8):
    """t [rows, C] as a column slice of a wider buffer (row stride C + pad)."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, device=t.device, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


# ------------------------------------------------------------------------------------ 1. footprint
def _mask(kind, n, H, W):
    if kind == "rect":
        return torch.from_numpy(FC.masks(f"fp{H}x{W}", n, H, W))
    m = torch.zeros(n, H, W, dtype=torch.int64)
    if kind == "allfg":
        m[:] = 1
    elif kind == "corner":
        m[:, H - 1, W - 1] = 1
    elif kind == "nofg":
        m[:, : max(H // 3, 1)] = 255
    return m


@pytest.mark.parametrize("kind", ["rect", "allfg", "nofg", "corner"])
@pytest.mark.parametrize("n,hs,ws,H,W", [(1, 1, 1, 1, 1), (2, 3, 4, 96, 128), (2, 3, 5, 50, 77), (1, 15, 20, 480, 640)])
def test_mask_footprint_vs_interpolate_adjoint(n, hs, ws, H, W, kind):
    from dformer_amd import kernels as K
    mask = _mask(kind, n, H, W)
    ind = torch.stack([mask == 0, mask == 1], 1).double()
    x = torch.zeros(n, 2, hs, ws, dtype=torch.float64, requires_grad=True)
    (F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False) * ind).sum().backward()
    foot, count = K.fss_mask_footprint(mask.to(DEV), (hs, ws))
    foot2, count2 = K.fss_mask_footprint(mask.to(DEV), (hs, ws))
    torch.cuda.synchronize()
    assert torch.equal(count.cpu().double(), ind.sum((2, 3)))  # exact
    scale = max(x.grad.abs().max().item(), 1.0)
    e = ((foot.cpu().double() - x.grad).abs().max() / scale).item()
    tot = foot.double().sum((2, 3)).cpu()
    e_sum = ((tot - count.cpu().double()).abs() / count.cpu().double().clamp_min(1.0)).max().item()
    print(f"footprint {(n, hs, ws, H, W)} {kind}: foot {e:.2e} sum-vs-count {e_sum:.2e}")
    assert e < 1e-4 and e_sum < 1e-6
    assert torch.equal(foot, foot2) and torch.equal(count, count2)  # fixed-order sums
    if kind == "nofg":
        assert torch.count_nonzero(count[:, 1]) == 0 and torch.count_nonzero(foot[:, 1]) == 0
    if kind == "corner":
        assert torch.equal(count[:, 1].cpu(), torch.ones(n)) and foot[0, 1, hs - 1, ws - 1].item() == 1.0


# --------------------------------------------------------------- 2. prototype pool and similarity
def _pool_inputs(B, S, cells, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    n = B * S
    f = torch.randn(n * cells, C, generator=g).to(dtype)
    foot = torch.rand(n, 2, cells, generator=g) * 50.0
    foot[:, :, ::3] = 0.0  # cells outside a class's footprint
    count = foot.sum(-1) * (1.0 + 0.1 * torch.rand(n, 2, generator=g))
    return f, foot, count


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,cells,C", [(1, 1, 1, 8), (2, 2, 12, 64), (2, 5, 300, 512), (1, 3, 35, 96)])
def test_proto_pool_fwd_bwd(B, S, cells, C, dtype):
    from dformer_amd import kernels as K
    f, foot, count = _pool_inputs(B, S, cells, C, dtype, 100 * cells + C)
    f64 = f.double().view(B * S, cells, C).requires_grad_()
    want = FC.proto64(f64, foot.double(), count.double(), B, S)
    dproto = torch.randn(B, 2, C, generator=torch.Generator().manual_seed(1))
    (df64,) = torch.autograd.grad(want, f64, dproto.double())
    fd = strided(f.to(DEV))
    proto, wgt = K.fss_proto_pool_fwd(fd, foot.to(DEV), count.to(DEV), B, S)
    df = K.fss_proto_pool_bwd(wgt, dproto.to(DEV), B, S, dtype)
    proto2, _ = K.fss_proto_pool_fwd(fd, foot.to(DEV), count.to(DEV), B, S)
    torch.cuda.synchronize()
    assert proto.dtype == torch.float32 and df.dtype == dtype
    e_p, e_d = rel_err(proto.cpu(), want.detach()), rel_err(df.float().cpu(), df64.view(-1, C))
    print(f"pool {(B, S, cells, C)} {dtype}: proto {e_p:.2e} df {e_d:.2e}")
    assert e_p < 1e-4 and e_d < tol_of(dtype)
    assert torch.equal(proto, proto2)


@pytest.mark.parametrize("T", [1.0, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,cells,C", [(1, 1, 1, 8), (2, 2, 12, 64), (2, 5, 300, 512), (1, 3, 35, 96)])
def test_similarity_fwd_bwd(B, S, cells, C, dtype, T):
    from dformer_amd import kernels as K
    g = torch.Generator().manual_seed(7 * cells + C)
    q = torch.randn(B * cells, C, generator=g).to(dtype)
    proto = torch.randn(B, 2, C, generator=g) + 0.5 * q.float().view(B, cells, C)[:, :1]  # correlated with a row
    dprob = torch.randn(B * cells, 2, generator=g)
    dq0 = torch.randn(B * cells, C, generator=g).to(dtype)
    q64 = q.double().view(B, cells, C).requires_grad_()
    p64 = proto.double().requires_grad_()
    cos = F.cosine_similarity(q64[:, :, None, :], p64[:, None, :, :], dim=-1)  # [B, cells, 2], eps 1e-8
    want = torch.softmax(20.0 * cos / T, -1)
    dq64, dp64 = torch.autograd.grad(want, [q64, p64], dprob.double().view(B, cells, 2))
    qd, pd = strided(q.to(DEV)), proto.to(DEV)
    prob, saved = K.fss_sim_fwd(qd, pd, T)
    dq, dproto = K.fss_sim_bwd(qd, pd, dprob.to(DEV), prob, saved, T)
    acc = strided(dq0.to(DEV).clone())
    dq_acc, dproto2 = K.fss_sim_bwd(qd, pd, dprob.to(DEV), prob, saved, T, dq=acc, accumulate=True)
    prob_i, saved_i = K.fss_sim_fwd(qd, pd, T, save=False)
    torch.cuda.synchronize()
    tol = tol_of(dtype)
    errs = {"prob": rel_err(prob.cpu(), want.detach().view(-1, 2)), "dproto": rel_err(dproto.cpu(), dp64),
            "dq": rel_err(dq.float().cpu(), dq64.view(-1, C)),
            "dq+": rel_err(dq_acc.float().cpu(), dq64.view(-1, C) + dq0.double())}
    print(f"sim {(B, cells, C)} {dtype} T={T}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["prob"] < 1e-4 and errs["dproto"] < 1e-4 and errs["dq"] < tol and errs["dq+"] < tol, errs
    assert dq_acc.data_ptr() == acc.data_ptr() and dq.dtype == dtype
    assert torch.equal(dproto, dproto2) and torch.equal(prob_i, prob) and saved_i[0] is None  # bit-identical rerun


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_prototype(dtype):
    """Episode 0 has no foreground pixel in any shot: its fg prototype is exactly zero, so sim = 0 exactly
    (prob = softmax(20 cos_bg / T, 0)), everything stays finite and the support rows get an exactly zero gradient
    from the empty class. dproto of the zero prototype is not compared (torch versions differ below the clamp)."""
    from dformer_amd import kernels as K
    B, S, cells, C = 2, 2, 12, 64
    f, foot, count = _pool_inputs(B, S, cells, C, dtype, 3)
    foot[:S, 1] = 0.0
    count[:S, 1] = 0.0
    proto, wgt = K.fss_proto_pool_fwd(f.to(DEV), foot.to(DEV), count.to(DEV), B, S)
    assert torch.count_nonzero(proto[0, 1]) == 0 and torch.count_nonzero(proto[0, 0]) > 0
    q = torch.randn(B * cells, C).to(dtype).to(DEV)
    prob, (cos, qn, pn) = K.fss_sim_fwd(q, proto, 1.0)
    assert torch.count_nonzero(cos[:cells, 1]) == 0 and torch.isfinite(prob).all()
    want = torch.softmax(torch.stack([20.0 * cos[:cells, 0], torch.zeros_like(cos[:cells, 0])], -1), -1)
    assert rel_err(prob[:cells].cpu(), want.cpu()) < 1e-6
    dq, dproto = K.fss_sim_bwd(q, proto, torch.randn(B * cells, 2, device=DEV), prob, (cos, qn, pn), 1.0)
    assert torch.isfinite(dq.float()).all() and torch.isfinite(dproto).all()
    only_fg = torch.zeros(B, 2, C, device=DEV)
    only_fg[:, 1] = dproto[:, 1]
    df = K.fss_proto_pool_bwd(wgt, only_fg, B, S, dtype)
    assert torch.count_nonzero(df[:S * cells]) == 0 and torch.count_nonzero(df[S * cells:]) > 0


# ------------------------------------------------------------------------------ 3. dual-source loss
LOSS_SHAPES = [(1, 1, 1, 1, 1, 1, 1), (2, 12, 16, 3, 4, 96, 128), (2, 7, 9, 2, 3, 50, 77), (1, 60, 80, 15, 20, 480, 640)]


def _loss_inputs(shape, dtype, ignore_all=False):
    B, h, w, hs, ws, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    low = (torch.randn(B, h, w, 2, generator=g) * 2.0).to(dtype)
    prob = torch.softmax(torch.randn(B, hs, ws, 2, generator=g) * 2.0, -1)
    lab = torch.from_numpy(FC.masks(f"loss{H}x{W}", B, H, W))
    if H * W == 1:
        lab[:] = 1  # the 255 band would cover the only pixel
    if ignore_all:
        lab[:] = 255
    return low, prob, lab


def _loss64(low, prob, lab, alpha):
    l64 = low.double().requires_grad_()
    p64 = prob.double().requires_grad_()
    size = lab.shape[-2:]
    up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False)  # noqa: E731
    fused = alpha * up(l64) + (1.0 - alpha) * up(p64)
    if (lab != 255).any():
        loss = F.cross_entropy(fused, lab, ignore_index=255, reduction="none")[lab != 255].mean()
    else:
        loss = fused.sum() * 0.0
    dl, dp = torch.autograd.grad(loss, [l64, p64])
    return loss.item(), dl, dp, fused.detach()


def _run_loss(low, prob, lab, alpha, dtype):
    from dformer_amd import kernels as K
    B, h, w, _ = low.shape
    hs, ws = prob.shape[1:3]
    rows, pr, lb = low.to(DEV).view(-1, 2), prob.to(DEV).view(-1, 2), lab.to(DEV)
    out, gplane = K.fss_loss_fwd(rows, B, h, w, pr, hs, ws, lb, alpha)
    dl, dp = K.fss_loss_bwd(gplane, B, h, w, hs, ws, out, alpha, dtype)
    return out, dl, dp


@pytest.mark.parametrize("alpha", [0.5, 0.0, 1.0])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_dual_loss_vs_fp64(shape, alpha):
    from dformer_amd import kernels as K
    low, prob, lab = _loss_inputs(shape, torch.float32)
    loss64, dl64, dp64, fused64 = _loss64(low, prob, lab, alpha)
    out, dl, dp = _run_loss(low, prob, lab, alpha, torch.float32)
    out2, dl2, dp2 = _run_loss(low, prob, lab, alpha, torch.float32)
    B, h, w, hs, ws, H, W = shape
    fused = K.fss_fuse(low.to(DEV).view(-1, 2), B, h, w, prob.to(DEV).view(-1, 2), hs, ws, (H, W), alpha)
    torch.cuda.synchronize()
    assert out[1].item() == float((lab != 255).sum())
    loss = (out[0] / out[1].clamp_min(1.0)).item()
    e = {"loss": abs(loss - loss64) / abs(loss64), "fused": rel_err(fused.view(B, H, W, 2).permute(0, 3, 1, 2).cpu(), fused64)}
    if alpha > 0.0:
        e["dL"] = rel_err(dl.cpu().view(B, h, w, 2), dl64)
    else:
        assert torch.count_nonzero(dl) == 0  # exactly zero
    if alpha < 1.0:
        e["dprob"] = rel_err(dp.cpu().view(B, hs, ws, 2), dp64)
    else:
        assert torch.count_nonzero(dp) == 0
    print(f"dual loss {shape} alpha={alpha}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v < 1e-4 for v in e.values()), e
    assert torch.equal(out, out2) and torch.equal(dl, dl2) and torch.equal(dp, dp2)  # bit-identical second run
    if alpha == 1.0:  # the single-source fused loss on the same logits
        rows, lb = low.to(DEV).view(-1, 2), lab.to(DEV)
        ref = K.seg_loss_fwd(rows, B, h, w, 2, lb)
        dref = K.seg_loss_bwd(rows, B, h, w, 2, lb, ref)
        e1 = abs(loss - (ref[0] / ref[1].clamp_min(1.0)).item()) / abs(loss64)
        e2 = rel_err(dl.cpu(), dref.cpu())
        print(f"dual loss {shape} alpha=1 vs seg_loss: loss {e1:.2e} dL {e2:.2e}")
        assert e1 < 1e-6 and e2 < 1e-6


def test_dual_loss_bf16_logits_and_all_ignored():
    shape = LOSS_SHAPES[1]
    low, prob, lab = _loss_inputs(shape, torch.bfloat16)
    loss64, dl64, dp64, _ = _loss64(low, prob, lab, 0.5)
    out, dl, dp = _run_loss(low, prob, lab, 0.5, torch.bfloat16)
    assert dl.dtype == torch.bfloat16 and dp.dtype == torch.float32
    loss = (out[0] / out[1]).item()
    e = (abs(loss - loss64) / abs(loss64), rel_err(dl.float().cpu().view(dl64.shape), dl64),
         rel_err(dp.cpu().view(dp64.shape), dp64))
    print(f"dual loss bf16 logits: loss {e[0]:.2e} dL {e[1]:.2e} dprob {e[2]:.2e}")
    assert e[0] < 1e-4 and e[1] < BF16_TOL and e[2] < 1e-4
    low, prob, lab = _loss_inputs(shape, torch.float32, ignore_all=True)
    out, dl, dp = _run_loss(low, prob, lab, 0.5, torch.float32)
    assert out[0].item() == 0.0 and out[1].item() == 0.0
    assert torch.count_nonzero(dl) == 0 and torch.count_nonzero(dp) == 0


def test_accounting_tags():
    """The wrappers charge their launches to the component tag that is set, with non-zero algorithmic bytes."""
    from dformer_amd import kernels as K
    low, prob, lab = _loss_inputs(LOSS_SHAPES[1], torch.float32)
    K.ACCOUNT = []
    K.trace(1)
    try:
        K.TAG = "fss"
        foot, count = K.fss_mask_footprint(lab.to(DEV), (3, 4))
        out, gplane = K.fss_loss_fwd(low.to(DEV).view(-1, 2), 2, 12, 16, prob.to(DEV).view(-1, 2), 3, 4, lab.to(DEV), 0.5)
        K.TAG = "fss.bwd"
        K.fss_loss_bwd(gplane, 2, 12, 16, 3, 4, out, 0.5, torch.float32)
        torch.cuda.synchronize()
    finally:
        K.trace(0)
        acct, K.ACCOUNT = K.ACCOUNT, None
    assert [a[-1] for a in acct] == ["fss", "fss", "fss.bwd"] and all(a[2] > 0 for a in acct)
    names = [[K.kernel_name(f) for f in a[0]] for a in acct]
    assert len(names[0]) == 3 and "fss_adjoint_xpass_kernel" in names[0][0] and "fss_adjoint_ypass_kernel" in names[0][1]
    assert len(names[1]) == 2 and "fss_loss_fwd_kernel" in names[1][0]
    assert len(names[2]) == 4


# ------------------------------------------------------------------------------------ 4. the model
E = FC.E2E


def build(dt=torch.float32, **over):
    from dformer_amd.encoder import Attention1Dto2D
    from dformer_amd.segmentor import EncoderDecoder
    g = load("e2e_fss_small")
    cfg = Cfg(backbone="DFormerTrav-Base", decoder="ham", decoder_embed_dim=512, num_classes=2, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, aux_rate=0, alpha=E["alpha"],
              temperature=E["temperature"])
    cfg.update(over)
    model = EncoderDecoder(cfg=cfg, syncbn=False)
    model.decode_head.dropout_ratio = 0.0
    model.encoder_backbone.attn_expand_e = Attention1Dto2D(E["N"], E["W"], E["H"], 64, 4)
    TC.load_values(model, int(g["wmeta"][0]), float(g["wmeta"][1]))
    return model.cuda().set_compute_dtype(dt), g


def episode(g, empty=()):
    B, S, H, W, N, seed, mseed = [int(v) for v in g["meta"]]
    rgb, _ = gen.rgb_depth(B * S + B, H, W, seed=seed)
    x = TC.scans("e2e_fss_small", B * S + B, N)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().cuda()  # noqa: E731
    bases = torch.from_numpy(gen.nmf_bases(B, 512, 64, name="e2e_fss_small/bases")).float()
    return dict(s_rgb=t(rgb[:B * S]).view(B, S, 3, H, W), s_depth=t(x[:B * S]).view(B, S, 1, N),
                s_mask=torch.from_numpy(FC.masks("e2e_fss_small", B * S, H, W, seed=mseed, empty=empty)).cuda()
                .view(B, S, H, W), q_rgb=t(rgb[B * S:]), q_depth=t(x[B * S:]).view(B, 1, N),
                q_gt=torch.from_numpy(FC.masks("e2e_fss_small/q", B, H, W)).cuda()), bases


def _train_forward(model, ep, bases):
    model.train()
    model.decode_head.hamburger.ham.injected_bases = bases
    model.return_logits = False
    model.keep_episode = True
    return model.meta_forward(ep["s_rgb"], ep["s_depth"], ep["s_mask"], ep["q_rgb"], ep["q_depth"], ep["q_gt"])


@pytest.fixture(scope="module")
def fp32_episode():
    """One float32 training episode of the golden's model, forward + backward: shared, left unchanged."""
    model, g = build()
    ep, bases = episode(g)
    loss, low = _train_forward(model, ep, bases)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    last = {k: v.clone() for k, v in model.last_episode.items()}
    return g, loss.item(), low.detach().float().clone(), last, grads


def gate(g, key):
    return max(1e-4, 10.0 * float(g["env/" + key]))


def test_meta_forward_fp32_vs_reference(fp32_episode):
    g, loss, low, last, grads = fp32_episode
    assert tuple(low.shape) == tuple(g["low"].shape) == (2, 2, 12, 16)
    e = {"proto": rel_err(last["proto"].cpu(), g["proto"]), "prob": rel_err(last["prob"].cpu(), g["prob"]),
         "low": rel_err(low.cpu(), g["low"]), "loss": abs(loss - float(g["loss"])) / abs(float(g["loss"]))}
    print("e2e_fss_small fp32: " + " ".join(f"{k} {v:.2e} (gate {gate(g, k):.1e})" for k, v in e.items()))
    assert all(v < gate(g, k) for k, v in e.items()), e
    bad, seen_fp, worst = [], 0, 0.0
    env = dict(zip(g["gfp_keys"].tolist(), g["env/gfp"].tolist()))  # the reference's own float32 error, per key
    for k, v in g.items():
        if k.startswith("gfp/"):
            seen_fp += 1
            err = fp_rel_err(gen.fingerprint(grads[k[4:]].cpu().double().numpy(), 16), v, atol=1e-4)
            tol = max(1e-4, 10.0 * env[k[4:]])
            worst = max(worst, err / tol)
            if err > tol:
                bad.append((k, err, env[k[4:]]))
    print(f"e2e_fss_small fp32: {seen_fp} gradient fingerprints, worst error / gate {worst:.2f}")
    assert seen_fp > 300 and not bad, bad[:10]
    # the support images reach the encoder: the stem weight's gradient is the golden's, and it is not zero
    stem = "encoder_backbone.downsample_layers.0.0.weight"
    assert np.abs(g["gfp/" + stem][:3]).min() > 0 and torch.count_nonzero(grads[stem]) > 0


def test_meta_forward_eval_and_empty_class(fp32_episode):
    g = fp32_episode[0]
    model, _ = build()
    ep, bases = episode(g)
    model.eval()
    model.decode_head.hamburger.ham.injected_bases = bases
    with torch.no_grad():
        out = model.meta_forward(ep["s_rgb"], ep["s_depth"], ep["s_mask"], ep["q_rgb"], ep["q_depth"])
    assert tuple(out.shape) == (2, 2, E["H"], E["W"]) and out.dtype == torch.float32
    e = rel_err(out.cpu(), g["fused_eval"])
    print(f"e2e_fss_small eval fused logits {e:.2e} (gate {gate(g, 'fused_eval'):.1e})")
    assert e < gate(g, "fused_eval")
    model2, _ = build()
    ep2, _ = episode(g, empty=(1,))
    with torch.no_grad():
        loss, _ = _train_forward(model2, ep2, bases)
    last = model2.last_episode
    e2 = {"proto": rel_err(last["proto"].cpu(), g["proto_empty"]), "prob": rel_err(last["prob"].cpu(), g["prob_empty"]),
          "loss": abs(loss.item() - float(g["loss_empty"])) / abs(float(g["loss_empty"]))}
    print("e2e_fss_small, support image 1 without foreground: " + " ".join(f"{k} {v:.2e}" for k, v in e2.items()))
    assert all(v < gate(g, k) for k, v in e2.items()), e2
    assert last["count"][1, 1].item() == 0.0


def _tail(f3, low, foot, count, q_gt, B, S):
    """The few-shot tail alone, forward + backward, on leaves f3 [n, C, hs, ws] and low [B, 2, h, w]."""
    from dformer_amd.decoders import FssLossFn, FssProtoSimFn, _nhwc_rows
    f3, low = f3.detach().requires_grad_(), low.detach().requires_grad_()
    hs, ws = f3.shape[-2:]
    _, prob, proto = FssProtoSimFn.apply(f3, foot, count, B, S, E["temperature"])
    rows, (_, h, w) = _nhwc_rows(low)
    loss = FssLossFn.apply(rows, prob, B, h, w, hs, ws, q_gt, E["alpha"])
    df3, dlow = torch.autograd.grad(loss, [f3, low])
    return dict(proto=proto, prob=prob, loss=loss.detach().reshape(1), df3=df3.float(), dlow=dlow.float())


def test_meta_forward_bf16_vs_fp32_run(fp32_episode):
    """bf16 compute. The per-module rule (1e-2 rel-to-max, a module against its float32 self on the same
    inputs) is asserted on the module this file adds: the few-shot tail on the bf16 run's own stage-3 map and
    logits, in bf16 and in float32. The figures against the float32 run of the whole model are printed only:
    they carry the encoder's and the decode head's bf16 error (tests/test_segmentor_gpu.py gates those against
    the reference's own bf16 envelope; a flat 1e-2 end to end is missed by the reference's autocast itself)."""
    g, loss32, low32, last32, _ = fp32_episode
    model, _ = build(torch.bfloat16)
    ep, bases = episode(g)
    seen = {}
    encode = model.encode
    model.encode = lambda rgb, x: seen.setdefault("feats", encode(rgb, x))
    loss, low = _train_forward(model, ep, bases)
    loss.backward()
    torch.cuda.synchronize()
    last = model.last_episode
    f3 = seen["feats"][-1]
    assert low.dtype == f3.dtype == torch.bfloat16 and torch.equal(last["foot"], last32["foot"])
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    e = {"proto": rel_err(last["proto"].cpu(), last32["proto"].cpu()), "prob": rel_err(last["prob"].cpu(), last32["prob"].cpu()),
         "low": rel_err(low.float().cpu(), low32.cpu()), "loss": abs(loss.item() - loss32) / abs(loss32)}
    print("e2e_fss_small bf16 vs fp32 run, whole model: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    B, S = E["B"], E["S"]
    t16 = _tail(f3, low, last["foot"], last["count"], ep["q_gt"], B, S)
    t32 = _tail(f3.float(), low.float(), last["foot"], last["count"], ep["q_gt"], B, S)
    assert torch.equal(t16["proto"], last["proto"]) and t16["loss"].item() == loss.item()  # the model ran this tail
    e = {k: rel_err(t16[k].cpu(), t32[k].cpu()) for k in t16}
    print("e2e_fss_small bf16 tail vs float32 tail on the same inputs: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v < 1e-2 for v in e.values()), e


# ------------------------------------------------------------------ 5. training step, evaluation, rejections
def _small_model(seed=3, **over):
    import bench
    from dformer_amd.encoder import Attention1Dto2D
    from dformer_amd.segmentor import EncoderDecoder
    cfg = bench.make_cfg("DFormer-Base", "ham")
    cfg.update(backbone="DFormerTrav-Base", drop_path_rate=0.0, num_classes=2, alpha=0.5, temperature=1.0)
    cfg.update(over)
    torch.manual_seed(seed)
    m = EncoderDecoder(cfg=cfg)
    m.encoder_backbone.attn_expand_e = Attention1Dto2D(24, 96, 64, 64, 4)
    m.decode_head.dropout_ratio = 0.0
    return cfg, m.cuda()


def _small_episode(B=1, S=2, H=64, W=96, N=24, name="step"):
    n = B * S + B
    rgb, _ = gen.rgb_depth(n, H, W, seed=5)
    x = torch.from_numpy(TC.scans(name, n, N)).float().cuda()
    rgb = torch.from_numpy(np.ascontiguousarray(rgb)).float().cuda()
    return (rgb[:B * S].view(B, S, 3, H, W), x[:B * S].view(B, S, 1, N),
            torch.from_numpy(FC.masks(name, B * S, H, W)).cuda().view(B, S, H, W), rgb[B * S:], x[B * S:].view(B, 1, N),
            torch.from_numpy(FC.masks(name + "/q", B, H, W)).cuda())


def test_meta_train_step_is_reproducible():
    from dformer_amd.train import FusedAdamW, meta_train_step
    ep = _small_episode()
    bases = torch.from_numpy(gen.nmf_bases(1, 512, 64, name="step/bases")).float().cuda()
    runs = []
    for _ in range(2):
        cfg, m = _small_model()
        m = m.set_compute_dtype(torch.bfloat16).train()
        m.return_logits = False
        m.decode_head.hamburger.ham.injected_bases = bases
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        opt = FusedAdamW(m, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
        losses = [meta_train_step(m, opt, *ep).item() for _ in range(2)]
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
        assert np.isfinite(losses).all() and opt.step_count == 2
        moved = [n for n, p in m.named_parameters() if not torch.equal(p.detach(), before[n])]
        assert "encoder_backbone.downsample_layers.0.0.weight" in moved and "decode_head.conv_seg.weight" in moved
    assert runs[0][0] == runs[1][0]
    for n, p in runs[0][1].items():
        assert torch.equal(p, runs[1][1][n]), n


def test_fss_evaluate_counts_meta_forward_argmax():
    from dformer_amd import evaluate as Ev
    cfg, m = _small_model()
    m.eval()
    m.decode_head.hamburger.ham.injected_bases = torch.from_numpy(gen.nmf_bases(1, 512, 64, name="ev/bases")).float()
    eps = [_small_episode(name="ev0"), _small_episode(name="ev1")]
    loader = [dict(s_img=e[0], s_depth=e[1], s_gt=e[2], q_img=e[3], q_depth=e[4], q_gt=e[5], fn=["a.png"]) for e in eps]
    want = Ev.Metrics(2, 255, DEV)
    for e in eps:
        with torch.no_grad():
            out = m.meta_forward(*e[:5])
        onehot = F.one_hot(out.argmax(1), 2).permute(0, 3, 1, 2).float()
        want.update(onehot, e[5])
    got = Ev.fss_evaluate(m, loader, Cfg(num_classes=2, background=255), DEV)
    assert got.index == 2 and torch.equal(got.hist, want.hist) and got.hist.sum() > 0


def test_meta_forward_rejections():
    ep = _small_episode()
    _, m = _small_model(num_classes=3)
    with pytest.raises(NotImplementedError, match="num_classes"):
        m.meta_forward(*ep)
    _, m = _small_model(aux_rate=0.4)
    with pytest.raises(NotImplementedError, match="aux"):
        m.meta_forward(*ep)
    cfg, m = _small_model()
    del cfg["alpha"]
    with pytest.raises(ValueError, match="alpha"):
        m.meta_forward(*ep)
