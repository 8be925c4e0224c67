"""The DFormerTrav backbone on the GPU (DFormer.py:308-457): the two laser-expansion kernels against the
float64 collapse (trav_common), Attention1Dto2D and the whole model against the reference's float64 goldens
(oracle/golden_e2e.py), the depth stem's Cin = 1 input gradient, the optimizer / HIP-graph plumbing and
the evaluation surface with a scan as modal_x.

Tolerances: rel-to-max within max(1e-4, 10 x the reference's own float32 error stored in env/), the rule of
tests/test_aux_gpu.py. The kernel cases have no env entry: 1e-4. A quantity whose float64 value is
mathematically zero (the variance of a constant scan or a single beam, and with it dalpha) is compared against
the scale it has when the variance is of the order of the ranges' squares: max x^2 for var, B * max|ds| *
max|g| * max x^2 for dalpha. dc, a sum that may cancel, is compared against sum|ds|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
import trav_common as TC
from goldens import fp_rel_err, load, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.manual_seed(0)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def close(a, b, tol, floor=0.0):
    """max|a - b| <= tol * max(max|b|, floor); returns the error relative to that scale."""
    a, b = a.double().cpu(), b.double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / max(b.abs().max().item(), floor, 1e-300)).item()


# ----------------------------------------------------------------------------- 1. kernels vs float64
def _scan(kind, B, N, rng):
    x = rng.uniform(0.5, 10.0, (B, N))
    if kind == "constant":
        x[:] = 3.3
    elif kind == "outlier":
        x = rng.uniform(1.0, 3.0, (B, N))
        x[:, N // 2] = 60.0
    return torch.from_numpy(x)


@pytest.mark.parametrize("kind", ["uniform", "constant", "outlier"])
@pytest.mark.parametrize("B,N,L,Hh,Hout", [(1, 1, 1, 1, 1), (3, 12, 10, 4, 6), (2, 67, 37, 4, 5), (2, 360, 640, 4, 8)])
def test_kernels_vs_fp64_collapse(B, N, L, Hh, Hout, kind):
    from dformer_amd import kernels as K
    rng = np.random.default_rng(1000 * N + L)
    x = _scan(kind, B, N, rng)
    alpha = torch.from_numpy(rng.standard_normal((L, Hh)) * 1.5)  # both signs; |alpha| * std(x) up to ~15
    g = torch.from_numpy(rng.uniform(0.3, 1.0, Hh) * rng.choice([-1.0, 1.0], Hh))
    c = torch.tensor(0.7, dtype=torch.float64)
    dplane = torch.from_numpy(rng.standard_normal((B, Hout, L)))
    xf, af, gf, cf = x.float().to(DEV), alpha.float().to(DEV), g.float().to(DEV), c.float().reshape(1).to(DEV)
    # the float64 collapse of the SAME float32 inputs
    s64, mean64, var64 = TC.collapse64(xf.cpu().double(), af.cpu().double(), gf.cpu().double(), cf.cpu().double()[0])
    dpf = dplane.float().to(DEV)
    ds64, da64, dg64, dc64 = TC.collapse_grads64(dpf.cpu().double(), gf.cpu().double(), mean64, var64)

    plane, s, mean, var = K.laser_expand_fwd(xf, af, gf, cf, Hout)
    ds, dalpha, dg, dc = K.laser_expand_bwd(dpf, gf, mean, var)
    torch.cuda.synchronize()
    assert tuple(plane.shape) == (B, Hout, L) and plane.dtype == torch.float32
    assert torch.equal(plane, s[:, None, :].expand(B, Hout, L))  # constant along H, bitwise
    errs = {"s": close(s, s64, 1e-4), "mean": close(mean, mean64, 1e-4),
            "var": close(var, var64, 1e-4, floor=float(x.max()) ** 2 if kind == "constant" or N == 1 else 0.0),
            "ds": close(ds, ds64, 1e-4), "dg": close(dg, dg64, 1e-4), "dc": close(dc.reshape(()), dc64, 1e-4,
                                                                                   floor=ds64.abs().sum().item()),
            "dalpha": close(dalpha, da64, 1e-4,
                            floor=B * ds64.abs().max().item() * g.abs().max().item() * float(x.max()) ** 2
                            if kind == "constant" or N == 1 else 0.0)}
    print(f"laser kernels {(B, N, L, Hh, Hout)} {kind}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < 1e-4 for v in errs.values()), errs
    if kind == "constant" or N == 1:
        assert close(mean, x.float()[:, :1, None].expand(B, L, Hh), 1e-6) < 1e-6
    # inference: no moments, the same plane
    plane_i, s_i, m_i, v_i = K.laser_expand_fwd(xf, af, gf, cf, Hout, save=False)
    assert m_i is None and v_i is None and torch.equal(plane_i, plane) and torch.equal(s_i, s)
    # fixed-order sums: a second run of each kernel is bit-identical
    plane2, s2, mean2, var2 = K.laser_expand_fwd(xf, af, gf, cf, Hout)
    out2 = K.laser_expand_bwd(dpf, gf, mean, var)
    assert torch.equal(plane2, plane) and torch.equal(s2, s) and torch.equal(mean2, mean) and torch.equal(var2, var)
    assert all(torch.equal(a, b) for a, b in zip(out2, (ds, dalpha, dg, dc)))


def test_kernels_other_head_counts_and_tracer_tag():
    """Hh = 3 (lanes of a column padded to 4; 600 (l, h) pairs: three gradient workgroups whose first head
    differs, 256 being no multiple of 3) and Hh = 8, and the launch accounting under tag `laser`."""
    from dformer_amd import kernels as K
    rng = np.random.default_rng(5)
    for Hh in (3, 8):
        B, N, L, Hout = 2, 19, 200, 3
        x, alpha = _scan("uniform", B, N, rng), torch.from_numpy(rng.standard_normal((L, Hh)))
        g, c = torch.from_numpy(rng.uniform(0.3, 1.0, Hh)), torch.tensor(-0.2, dtype=torch.float64)
        xf, af, gf, cf = x.float().to(DEV), alpha.float().to(DEV), g.float().to(DEV), c.float().reshape(1).to(DEV)
        s64, mean64, var64 = TC.collapse64(xf.cpu().double(), af.cpu().double(), gf.cpu().double(), cf.cpu().double()[0])
        dpf = torch.from_numpy(rng.standard_normal((B, Hout, L))).float().to(DEV)
        want = TC.collapse_grads64(dpf.cpu().double(), gf.cpu().double(), mean64, var64)
        plane, s, mean, var = K.laser_expand_fwd(xf, af, gf, cf, Hout)
        got = K.laser_expand_bwd(dpf, gf, mean, var)
        assert close(s, s64, 1e-4) < 1e-4 and torch.equal(plane, s[:, None, :].expand(B, Hout, L))
        for a, b in zip(got, want):
            assert close(a.reshape(b.shape), b, 1e-4) < 1e-4, Hh
    K.ACCOUNT = []
    K.trace(1)
    try:
        K.TAG = "laser"
        plane, s, mean, var = K.laser_expand_fwd(xf, af, gf, cf, Hout)
        K.laser_expand_bwd(dpf, gf, mean, var)
        torch.cuda.synchronize()
    finally:
        K.trace(0)
        acct, K.ACCOUNT = K.ACCOUNT, None
    assert [a[-1] for a in acct] == ["laser", "laser"] and all(a[1] > 0 and a[2] > 0 and a[3] == "f32" for a in acct)
    names = [[K.kernel_name(f) for f in a[0]] for a in acct]
    assert len(names[0]) == 1 and "laser_expand_fwd_kernel" in names[0][0]
    assert len(names[1]) == 3 and "laser_rowsum_kernel" in names[1][0] and "laser_param_grad_kernel" in names[1][1]
    assert "laser_param_grad_final_kernel" in names[1][2]
    with pytest.raises(RuntimeError, match="exceeds the 8192"):
        K.laser_expand_fwd(torch.zeros(1, 8193, device=DEV), af, gf, cf, Hout)


# --------------------------------------------------------------------- 2. the module vs the reference
def _expand_module(g):
    from dformer_amd.encoder import Attention1Dto2D
    from dformer_amd.functional import invalidate_weights
    B, N, L, Hout = [int(v) for v in g["meta"]]
    mod = TC.load_values(Attention1Dto2D(N, L, Hout, 64, 4), int(g["wmeta"][0]), float(g["wmeta"][1]))
    invalidate_weights()
    return mod.cuda(), (B, N, L, Hout)


@pytest.mark.parametrize("name", ["trav_expand_small", "trav_expand_full"])
def test_attention1dto2d_vs_reference(name):
    g = load(name)
    mod, (B, N, L, Hout) = _expand_module(g)
    x = torch.from_numpy(TC.scans(name, B, N)).float().cuda().unsqueeze(1)
    plane = mod(x)
    assert tuple(plane.shape) == (B, 1, Hout, L) and plane.dtype == torch.float32
    assert torch.equal(plane, plane[:, :, :1].expand_as(plane))
    plane.backward(torch.from_numpy(gen.normal(name + "/gy", (B, 1, Hout, L))).float().cuda())
    e = rel_err(plane[:, 0, 0].detach().cpu(), g["s"])
    tol = max(1e-4, 10.0 * float(g["env/s"]))
    print(f"{name}: s {e:.2e} (tol {tol:.1e})")
    assert e < tol
    grads = {n: p.grad for n, p in mod.named_parameters()}
    assert all(v is not None for v in grads.values()) and len(grads) == 14
    for k, v in TC.zero_parts(grads).items():
        assert torch.count_nonzero(v) == 0, k  # exact zeros, not rounding noise
    worst = {}
    for n, gr in grads.items():
        ref = g["grad/" + n]
        if np.abs(ref).max() == 0:
            assert torch.count_nonzero(gr) == 0, n
            continue
        worst[n] = (rel_err(gr.cpu(), ref), max(1e-4, 10.0 * float(g["env/grad/" + n])))
    print(f"{name}: grads " + " ".join(f"{n} {e:.1e}" for n, (e, _) in worst.items()))
    assert len(worst) == 13 and not {n: v for n, v in worst.items() if v[0] >= v[1]}, worst
    # eval: the folded triple is cached until the weights change
    mod.eval()
    with torch.no_grad():
        p1 = mod(x)
        f1 = mod.folded()
        assert mod.folded()[0] is f1[0] and torch.equal(p1, plane)
        mod.output_proj.bias.add_(1.0)
        from dformer_amd.functional import invalidate_weights
        invalidate_weights()
        assert mod.folded()[0] is not f1[0]
        assert rel_err((mod(x) - p1).cpu(), torch.ones_like(p1).cpu()) < 1e-5


# ------------------------------------------------------------------------------------ 3. end to end
def build(dt=torch.float32):
    from dformer_amd.encoder import Attention1Dto2D
    from dformer_amd.segmentor import EncoderDecoder
    g = load("e2e_trav_small")
    B, H, W, ncls, seed, N = [int(v) for v in g["meta"]]
    cfg = Cfg(backbone="DFormerTrav-Base", decoder="ham", decoder_embed_dim=512, num_classes=ncls, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, aux_rate=0)
    model = EncoderDecoder(cfg=cfg, syncbn=False)
    model.decode_head.dropout_ratio = 0.0
    model.encoder_backbone.attn_expand_e = Attention1Dto2D(N, W, H, 64, 4)
    TC.load_values(model, int(g["wmeta"][0]), float(g["wmeta"][1]))
    return model.cuda().set_compute_dtype(dt), g


def _inputs(g):
    B, H, W, ncls, seed, N = [int(v) for v in g["meta"]]
    rgb_np, _ = gen.rgb_depth(B, H, W, seed=seed)
    bases = torch.from_numpy(gen.nmf_bases(B, 512, 64, name="e2e_trav_small/bases")).float()
    return (torch.from_numpy(rgb_np).float().cuda(), torch.from_numpy(TC.scans("e2e_trav_small", B, N)).float().cuda()
            .unsqueeze(1), torch.from_numpy(gen.labels(B, H, W, ncls)).cuda(), bases)


@pytest.fixture(scope="module")
def fp32_step():
    """One float32 training forward + backward of the golden's model: shared, left unchanged."""
    model, g = build()
    rgb, scan, lab, bases = _inputs(g)
    model.train()
    model.decode_head.hamburger.ham.injected_bases = bases
    model.return_logits = False
    seen = {}
    hook = model.encoder_backbone.attn_expand_e.register_forward_hook(
        lambda m, a, o: seen.__setitem__("plane", o.detach()))
    loss, low = model(rgb, scan, lab)
    loss.backward()
    hook.remove()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return g, loss.item(), low.detach().float().clone(), seen["plane"].clone(), grads


def test_model_fp32_vs_reference(fp32_step):
    g, loss, low, plane, grads = fp32_step
    assert tuple(low.shape) == tuple(g["low"].shape) == (2, 2, 8, 12)
    e_low, e_loss = rel_err(low.cpu(), g["low"]), abs(loss - float(g["loss"])) / abs(float(g["loss"]))
    print(f"e2e_trav_small fp32: low {e_low:.2e} loss {e_loss:.2e}")
    assert e_low < 1e-3 and e_loss < 1e-5
    bad, seen_fp, worst = [], 0, 0.0
    for k, v in g.items():
        if k.startswith("gfp/"):
            seen_fp += 1
            e = fp_rel_err(gen.fingerprint(grads[k[4:]].cpu().double().numpy(), 16), v, atol=1e-4)
            worst = max(worst, e / max(1e-4, 10.0 * float(g["env/" + k])))
            if e > max(1e-4, 10.0 * float(g["env/" + k])):  # fp32_gate of tests/test_segmentor_gpu.py
                bad.append((k, e, float(g["env/" + k])))
    print(f"e2e_trav_small fp32: {seen_fp} gradient fingerprints, worst error / gate {worst:.2f}")
    assert seen_fp > 300 and not bad, bad[:10]
    pre = "encoder_backbone.attn_expand_e."
    ex = {n[len(pre):]: v for n, v in grads.items() if n.startswith(pre)}
    assert len(ex) == 14
    for k, v in TC.zero_parts(ex).items():
        assert torch.count_nonzero(v) == 0, k


def test_model_bf16_vs_fp32_run(fp32_step):
    """bf16 compute: the expansion itself stays float32 (the same plane, bitwise) and the depth stem that
    reads it, the first module in bf16, stays within the per-module 1e-2 rel-to-max of the float32 run."""
    g, _, _, plane32, _ = fp32_step
    model, _ = build(torch.bfloat16)
    rgb, scan, lab, bases = _inputs(g)
    model.train()
    model.decode_head.hamburger.ham.injected_bases = bases
    model.return_logits = False
    seen = {}
    bb = model.encoder_backbone
    bb.attn_expand_e.register_forward_hook(lambda m, a, o: seen.__setitem__("plane", o.detach()))
    loss, low = model(rgb, scan, lab)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(seen["plane"], plane32) and low.dtype == torch.bfloat16 and np.isfinite(loss.item())
    from dformer_amd.encoder import _run_downsample_native
    with torch.no_grad():
        bb.eval()
        e16 = _run_downsample_native(bb.downsample_layers_e[0], plane32, torch.bfloat16)
        e32 = _run_downsample_native(bb.downsample_layers_e[0], plane32, torch.float32)
    e = rel_err(e16.float().cpu(), e32.cpu())
    print(f"bf16 depth stem on the plane vs fp32: {e:.2e}")
    assert e < 1e-2
    assert all(torch.isfinite(p.grad).all() for p in bb.attn_expand_e.parameters())


# ------------------------------------------------------------------ 4. the depth stem's Cin = 1 dgrad
@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)])
def test_conv_s2_cin1_input_gradient(dt, tol):
    """ConvS2Fn without a folded BN on a 1-channel 8 x 12 plane (the first depth-stem conv, whose input
    gradient now feeds the expansion) against F.conv2d autograd; tolerances of tests/test_conv_gpu.py."""
    from dformer_amd.encoder import ConvS2Fn
    from dformer_amd.functional import invalidate_weights
    conv = torch.nn.Conv2d(1, 16, 3, 2, 1).to(DEV)
    invalidate_weights()
    x = torch.randn(2, 1, 8, 12, device=DEV, requires_grad=True)
    y = ConvS2Fn.apply(x, conv.weight, conv.bias, None, None, None, False, False, dt)
    assert tuple(y.shape) == (2 * 4 * 6, 16) and y.dtype == dt
    dy = torch.randn(2 * 4 * 6, 16, device=DEV).to(dt)
    gx, gw, gb = torch.autograd.grad(y, [x, conv.weight, conv.bias], dy)
    xr = x.detach().clone().requires_grad_()
    ref = F.conv2d(xr, conv.weight, conv.bias, stride=2, padding=1)
    rx, rw, rb = torch.autograd.grad(ref, [xr, conv.weight, conv.bias],
                                     dy.float().view(2, 4, 6, 16).permute(0, 3, 1, 2))
    assert gx.dtype == torch.float32 and tuple(gx.shape) == (2, 1, 8, 12)
    assert rel_err(y.float().view(2, 4, 6, 16).permute(0, 3, 1, 2).cpu(), ref.detach().cpu()) < tol
    assert rel_err(gx.cpu(), rx.cpu()) < tol and rel_err(gw.cpu(), rw.cpu()) < tol and rel_err(gb.cpu(), rb.cpu()) < tol


# --------------------------------------------------------------------------- 5. training plumbing
NEVER_UPDATED = ["query1", "query2", "attn1.in_proj_weight", "attn1.in_proj_bias", "attn2.in_proj_weight",
                 "attn2.in_proj_bias"]


def test_graphed_steps_match_eager_and_respect_group_weight():
    """Trav-Base 2 x 64x96, bf16, FusedAdamW: two eager steps and two GraphedTrainStep replays agree bit for
    bit (the pattern of tests/test_graph_gpu.py); the parameters the reference's group_weight never collects
    stay as they were, input_proj.weight moves."""
    import bench
    from dformer_amd.encoder import Attention1Dto2D
    from dformer_amd.segmentor import EncoderDecoder
    from dformer_amd.train import FusedAdamW, GraphedTrainStep, train_step
    dev = torch.device("cuda", 0)

    def make():
        cfg = bench.make_cfg("DFormer-Base", "ham")
        cfg["backbone"] = "DFormerTrav-Base"
        cfg["drop_path_rate"] = 0.0
        cfg["num_classes"] = 2
        torch.manual_seed(3)
        m = EncoderDecoder(cfg=cfg)
        m.encoder_backbone.attn_expand_e = Attention1Dto2D(24, 96, 64, 64, 4)
        with torch.no_grad():
            m.encoder_backbone.attn_expand_e.query1.mul_(4.0)  # alpha of a few units: the queries matter
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
    rgb, _, lab = bench.synthetic_batch(2, 64, 96, cfg.num_classes, dev, 5)
    scan = torch.from_numpy(TC.scans("graph", 2, 24)).float().to(dev).unsqueeze(1)
    exp = dict(ma.encoder_backbone.attn_expand_e.named_parameters())
    before = {n: p.detach().clone() for n, p in exp.items()}
    la = [train_step(ma, oa, rgb, scan, lab).item() for _ in range(4)]
    for n in NEVER_UPDATED:
        assert torch.equal(exp[n].detach(), before[n]), n
    for n in ("input_proj.weight", "attn1.out_proj.weight", "attn2.out_proj.weight", "output_proj.weight"):
        assert not torch.equal(exp[n].detach(), before[n]), n
    g = GraphedTrainStep(mb, ob, rgb, scan, lab, warmup=2)
    lb = [g().item() for _ in range(2)]
    assert ob.step_count == oa.step_count == 4
    assert np.isfinite(la).all() and la[2:] == lb, (la, lb)
    for ga, gb_ in zip(oa.groups, ob.groups):
        assert torch.equal(ga.flat, gb_.flat) and torch.equal(ga.m, gb_.m) and torch.equal(ga.v, gb_.v)
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), n


# ----------------------------------------------------------------------------------- 6. evaluation
def test_predict_and_evaluate_with_laser_batches():
    """predict / evaluate / save-style class maps / evaluate_msf at scale 1 on a two-batch loader with the
    reference's `laser` key: the histogram is the bincount of forward's argmax."""
    from dformer_amd import evaluate as E
    model, g = build()
    rgb, scan, lab, bases = _inputs(g)
    model.decode_head.hamburger.ham.injected_bases = bases
    model.eval()
    ncls = 2
    # the second batch: the images swapped, the scans as the loader's [B, N] (no channel axis)
    batches = [(rgb, scan, lab), (rgb.flip(0), scan.flip(0)[:, 0], lab.flip(0))]
    loader = [dict(rgb=r, laser=s, gt=t) for r, s, t in batches]
    ref = torch.zeros(ncls * ncls, dtype=torch.int64, device=DEV)
    for r, s, t in batches:
        with torch.no_grad():
            out = model(r, s)
        assert tuple(out.shape) == (2, ncls, 64, 96)
        want = out.argmax(1)
        pred = model.predict(r, s)
        assert pred.dtype == torch.uint8 and torch.equal(pred.long(), want)
        keep = t != 255
        ref += torch.bincount(t[keep] * ncls + want[keep], minlength=ncls * ncls)
    cfg = Cfg(num_classes=ncls, background=255)
    m = E.evaluate(model, loader, cfg, DEV)
    assert m.index == 2 and torch.equal(m.hist.long().reshape(-1), ref)
    acc = E.msf_scores(model, rgb, scan, ncls, [1.0], False)
    with torch.no_grad():
        assert torch.equal(acc.view(2, 64, 96, ncls).argmax(-1), model(rgb, scan).argmax(1))
    mm = E.evaluate_msf(model, loader, cfg, DEV, [1.0], False)
    assert torch.equal(mm.hist, m.hist)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.evaluate_msf(model, loader, cfg, DEV, [0.75, 1.0], True)
    with pytest.raises(NotImplementedError, match="laser scan"):
        E.evaluate(model, loader, cfg, DEV, sliding=True)
