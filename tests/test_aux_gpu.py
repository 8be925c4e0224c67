"""The auxiliary FCN head on the GPU (fcnhead.py:9-29, builder.py:138-143, 204-207, 231-232): the dense 3x3
stride-1 gather / col2im kernels against torch, FCNHead against the reference's fp64 goldens
(oracle/golden_decoders.py / golden_e2e.py), the fused loss at the aux head's x16 / non-integer factors, the training forward
with aux_rate = 0.4 end to end, eval parity with a model without the head, and the optimizer / HIP-graph
plumbing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen
from goldens import check_param_grads, fp_rel_err, load, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # tests/test_conv_gpu.py's own
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.manual_seed(0)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _unfold_rows(x4):
    """F.unfold of NCHW x4 as gather rows [B*H*W, 9*C] in the library's (kh, kw, c) column order."""
    B, C, H, W = x4.shape
    u = F.unfold(x4, 3, padding=1).view(B, C, 9, H * W)  # columns (c, kh*3+kw)
    return u.permute(0, 3, 2, 1).reshape(B * H * W, 9 * C)


# ------------------------------------------------------------------ 1. gather / scatter vs torch
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cin", [128, 288])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (3, 2), (5, 7)])
@pytest.mark.parametrize("B", [1, 2])
def test_conv3s1_gather_scatter(dt, B, H, W, cin):
    from dformer_amd import kernels as K
    P, kp = B * H * W, 9 * cin
    assert K.conv3s2_kp(cin) == kp  # cin % 8 == 0: the Kp rule leaves no pad columns
    x = torch.randn(P, cin, device=DEV).to(dt)
    x4 = x.float().view(B, H, W, cin).permute(0, 3, 1, 2).contiguous().requires_grad_()
    ref_cols = _unfold_rows(x4)
    inside = _unfold_rows(torch.ones_like(x4)) > 0
    dcols = torch.randn(P, kp, device=DEV).to(dt)
    gref, = torch.autograd.grad(ref_cols, x4, dcols.float())
    gref = gref.permute(0, 2, 3, 1).reshape(P, cin)
    gtol = TOL[dt] * (2 if dt != torch.float32 else 1)
    for wide in (False, True):
        xs, sentinel = x, 7.0
        cols_buf = torch.full((P, kp + (8 if wide else 0)), sentinel, device=DEV, dtype=dt)
        dcs = dcols
        if wide:  # every operand a column slice of a wider buffer: row strides > Cin / 9*Cin
            xs = torch.full((P, cin + 16), 3.0, device=DEV, dtype=dt)[:, :cin]
            xs.copy_(x)
            dcs = torch.full((P, kp + 24), 5.0, device=DEV, dtype=dt)[:, :kp]
            dcs.copy_(dcols)
        cols = K.conv3s1_im2col(xs, (B, H, W), out=cols_buf[:, :kp])
        assert cols.shape == (P, K.conv3s2_kp(cin))
        assert rel(cols.float(), ref_cols.detach()) < TOL[dt]
        assert torch.all(cols[~inside] == 0)           # taps outside the image: exact zeros
        assert torch.all(cols[:, 9 * cin:] == 0)       # pad columns (none for cin % 8 == 0)
        assert torch.all(cols_buf[:, kp:] == sentinel)  # nothing written past a row's 9*Cin columns
        if not wide:
            assert torch.equal(K.conv3s1_im2col(xs, (B, H, W)), cols)
        for accumulate in (False, True):
            dx_buf = torch.randn(P, cin + (8 if wide else 0), device=DEV).to(dt)
            before = dx_buf.clone()
            dx = K.conv3s1_col2im(dcs, (B, H, W), cin, dx=dx_buf[:, :cin], accumulate=accumulate)
            want = gref + (before[:, :cin].float() if accumulate else 0)
            assert rel(dx.float(), want) < gtol, (wide, accumulate, rel(dx.float(), want))
            assert torch.equal(dx_buf[:, cin:], before[:, cin:])
            dx2_buf = before.clone()
            K.conv3s1_col2im(dcs, (B, H, W), cin, dx=dx2_buf[:, :cin], accumulate=accumulate)
            assert torch.equal(dx2_buf, dx_buf)        # fixed-order sum: bit-reproducible


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,W,cin,cout", [(2, 5, 7, 128, 37), (1, 3, 2, 288, 40), (2, 1, 5, 288, 37)])
def test_conv3s1_gemm_matches_conv2d(dt, B, H, W, cin, cout):
    """gather + packed-weight GEMM is nn.Conv2d(cin, cout, 3, padding=1), with its three gradients."""
    from dformer_amd import kernels as K
    conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV)
    x = torch.randn(B * H * W, cin, device=DEV).to(dt)
    x4 = x.float().view(B, H, W, cin).permute(0, 3, 1, 2).contiguous().requires_grad_()
    ref = F.conv2d(x4, conv.weight, conv.bias, padding=1)
    cols = K.conv3s1_im2col(x, (B, H, W))
    wp = K.conv3_weight_pack(conv.weight.detach(), dt, 9 * cin)
    y = K.linear(cols, wp, conv.bias.detach())
    assert rel(y.float().view(B, H, W, cout).permute(0, 3, 1, 2), ref.detach()) < TOL[dt]
    dy = torch.randn(B * H * W, cout, device=DEV).to(dt)
    gx, gw, gb = torch.autograd.grad(ref, [x4, conv.weight, conv.bias],
                                     dy.float().view(B, H, W, cout).permute(0, 3, 1, 2))
    tol = TOL[dt] * (2 if dt != torch.float32 else 1)
    dwp, db = K.linear_wgrad(dy, cols, bias_grad=True)
    assert rel(K.conv3_weight_unpack(dwp, cin), gw) < tol and rel(db, gb) < tol
    dx = K.conv3s1_col2im(K.linear_dgrad(dy, wp), (B, H, W), cin)
    assert rel(dx.float().view(B, H, W, cin).permute(0, 3, 1, 2), gx) < tol


# --------------------------------------------------------------------- 2. FCNHead vs the reference
def _fcn_head(g, dt=torch.float32):
    from dformer_amd.decoders import FCNHead
    from dformer_amd.functional import invalidate_weights
    B, cin, hidden, H, W, seed = [int(v) for v in g["meta"]]
    head = FCNHead(cin, hidden)
    sd = head.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    invalidate_weights()
    return head.cuda().train(), (B, cin, hidden, H, W), seed


@pytest.mark.parametrize("name", ["fcnhead_c128", "fcnhead_c288"])
def test_fcn_head_fp32_vs_reference(name):
    g = load(name)
    head, (B, cin, hidden, H, W), seed = _fcn_head(g)
    tag = f"{name}#{seed}"
    leaf = torch.from_numpy(gen.normal(tag + "/x", (B, cin, H, W))).float().cuda() \
        .permute(0, 2, 3, 1).contiguous().requires_grad_()
    y = head(leaf.permute(0, 3, 1, 2))
    assert tuple(y.shape) == (B, 40, H, W)  # the classifier is 40 wide whatever the hidden width
    y.backward(torch.from_numpy(gen.normal(tag + "/gy", tuple(y.shape))).float().cuda())
    assert rel_err(y.detach().cpu(), g["y"]) < 1e-4
    assert rel_err(leaf.grad.permute(0, 3, 1, 2).cpu(), g["gx"]) < 1e-3
    grads = {k: p.grad.cpu() for k, p in head.named_parameters()}
    # conv.0.bias sits ahead of a train-mode BN: its gradient is mathematically zero (the reference gives
    # ~1e-15), so it is out of the relative gates and only bounded against d conv.1.bias
    gated = {k: v for k, v in g.items() if k != "grad/conv.0.bias"}
    assert len([k for k in gated if k.startswith("grad/")]) == 5
    check_param_grads(gated, grads, 1e-3, atol=1e-6)
    b0 = grads["conv.0.bias"]
    assert torch.isfinite(b0).all() and b0.abs().max() < 1e-4 * np.abs(g["grad/conv.1.bias"]).max()
    bufs = dict(head.named_buffers())
    for k, v in g.items():
        if k.startswith("buf/"):
            assert rel_err(bufs[k[4:]].cpu(), v) < 1e-4, k
    assert int(bufs["conv.1.num_batches_tracked"]) == 1


@pytest.mark.parametrize("dt,key,floor", [(torch.bfloat16, "env_bf16/y", 2e-2), (torch.float16, "env_f16/y", 3e-3)])
@pytest.mark.parametrize("name", ["fcnhead_c128", "fcnhead_c288"])
def test_fcn_head_16bit_vs_reference_envelope(name, dt, key, floor):
    """Output within 1.5 x the reference's own autocast error on the same input (BF16_LOW of
    tests/test_segmentor_gpu.py), floored at the conv kernel's gate for the dtype."""
    g = load(name)
    head, (B, cin, hidden, H, W), seed = _fcn_head(g)
    x = torch.from_numpy(gen.normal(f"{name}#{seed}/x", (B, cin, H, W))).float().cuda()
    with torch.no_grad():
        y = head(x.permute(0, 2, 3, 1).contiguous().to(dt).permute(0, 3, 1, 2))
    assert y.dtype == dt
    e = rel_err(y.float().cpu(), g["y"])
    assert e <= max(1.5 * float(g[key]), floor), (e, float(g[key]))


@pytest.mark.parametrize("B,cin,hidden,H,W", [(2, 128, 37, 5, 7), (1, 288, 40, 3, 2)])
def test_fcn_head_eval_vs_torch(B, cin, hidden, H, W):
    """Eval mode: the running statistics, untouched, against torch's own conv / batch_norm in fp32."""
    from dformer_amd.decoders import FCNHead
    from dformer_amd.functional import invalidate_weights
    head = FCNHead(cin, hidden).cuda()
    bn = head.conv[1]
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    invalidate_weights()
    head.eval()
    run = (bn.running_mean.clone(), bn.running_var.clone())
    x = torch.randn(B, H, W, cin, device=DEV).requires_grad_()
    xr = x.detach().permute(0, 3, 1, 2).contiguous().requires_grad_()
    z = F.conv2d(xr, head.conv[0].weight, head.conv[0].bias, padding=1)
    z = F.relu(F.batch_norm(z, run[0], run[1], bn.weight, bn.bias, False, bn.momentum, bn.eps))
    ref = F.conv2d(z, head.classifier.weight, head.classifier.bias)
    y = head(x.permute(0, 3, 1, 2))
    assert rel(y, ref.detach()) < 1e-4
    assert torch.equal(bn.running_mean, run[0]) and torch.equal(bn.running_var, run[1])
    dy = torch.randn_like(ref)
    params = [head.conv[0].weight, head.conv[0].bias, bn.weight, bn.bias, head.classifier.weight,
              head.classifier.bias]
    g_ref = torch.autograd.grad(ref, [xr] + params, dy)
    g = torch.autograd.grad(y, [x] + params, dy)
    assert rel(g[0].permute(0, 3, 1, 2), g_ref[0]) < 1e-4
    for a, b in zip(g[1:], g_ref[1:]):
        assert rel(a, b) < 1e-4, a.shape


# ------------------------------------------------------------------- 3. the loss kernel on new ground
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,h,w,H,W", [(2, 4, 6, 64, 96), (2, 4, 5, 53, 73)])
def test_seg_loss_at_aux_factors(dt, B, h, w, H, W):
    """SegLossFn at the aux head's x16 and at a non-integer factor against F.interpolate +
    F.cross_entropy in fp64 (of the same, dtype-rounded logits), forward and gradient, at the tolerances
    tests/test_kernels_gpu.py uses for the existing loss cases: loss 1e-4, gradient 1e-3 rel-to-max, and
    4e-3 where the gradient is written in a 16-bit logits dtype (its test_seg_loss_fwd_grad_fused)."""
    from dformer_amd.decoders import SegLossFn
    ncls = 40
    lg = torch.randn(B * h * w, ncls, device=DEV).to(dt).requires_grad_()
    lab = torch.randint(0, ncls, (B, H, W), device=DEV)
    lab[torch.rand(B, H, W, device=DEV) < 0.1] = 255
    loss = SegLossFn.apply(lg, B, h, w, lab, 255)
    (loss * 3.0).backward()
    lr = lg.detach().double().view(B, h, w, ncls).permute(0, 3, 1, 2).contiguous().requires_grad_()
    up = F.interpolate(lr, (H, W), mode="bilinear", align_corners=False)
    ce = F.cross_entropy(up, lab, reduction="none", ignore_index=255)
    ref = ce[lab != 255].mean()
    (ref * 3.0).backward()
    assert abs(loss.item() - ref.item()) < 1e-4 * abs(ref.item()), (loss.item(), ref.item())
    assert lg.grad.dtype == dt
    e = rel(lg.grad.float().view(B, h, w, ncls).permute(0, 3, 1, 2), lr.grad)
    assert e < (1e-3 if dt == torch.float32 else 4e-3), e


# ------------------------------------------------------------------------------------ 4. end to end
def build(ncls, aux_rate=0.4):
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=ncls, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255)
    if aux_rate is not None:
        cfg["aux_rate"] = aux_rate
    model = EncoderDecoder(cfg=cfg, syncbn=False)
    model.decode_head.dropout_ratio = 0.0
    sd = model.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    return model.cuda()


def _inputs(g, ncls):
    B, H, W = [int(v) for v in g["meta"][:3]]
    rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=int(g["meta"][4]))
    bases = torch.from_numpy(gen.nmf_bases(B, 512, 64, name="e2e_tiny_small/bases")).float()
    return (torch.from_numpy(rgb_np).float().cuda(), torch.from_numpy(dep_np).float().cuda(),
            torch.from_numpy(gen.labels(B, H, W, ncls)).cuda(), bases)


@pytest.mark.parametrize("name,ncls", [("e2e_tiny_aux", 40), ("e2e_tiny_aux37", 37)])
def test_aux_training_forward_fp32_vs_reference(name, ncls):
    g = load(name)
    rgb, dep, lab, bases = _inputs(g, ncls)
    model = build(ncls).train()
    model.decode_head.hamburger.ham.injected_bases = bases
    seen = {}
    model.aux_head.register_forward_hook(lambda m, a, o: seen.__setitem__("aux_low", o.detach()))
    loss, out = model(rgb, dep, lab)
    loss.backward()
    torch.cuda.synchronize()
    aux_low = seen["aux_low"]
    assert tuple(aux_low.shape) == tuple(g["aux_low"].shape) == (2, 40, 4, 6)  # 40 wide with 37 classes too
    assert tuple(out.shape) == (2, ncls, 64, 96)
    assert rel_err(aux_low.float().cpu(), g["aux_low"]) < 1e-4
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    assert abs(float(g["loss"]) - (float(g["loss_main"]) + 0.4 * float(g["loss_aux"]))) < 1e-12
    named = dict(model.named_parameters())
    bad, seen_fp = [], 0
    for k, v in g.items():
        if k.startswith("gfp/"):
            seen_fp += 1
            e = fp_rel_err(gen.fingerprint(named[k[4:]].grad.cpu().double().numpy(), 16), v, atol=1e-4)
            if e > max(1e-4, 10.0 * float(g["env/" + k])):  # fp32_gate of tests/test_segmentor_gpu.py
                bad.append((k, e, float(g["env/" + k])))
    assert seen_fp > 200 and not bad, bad[:10]
    for k, v in g.items():
        if k.startswith("auxgrad/"):
            a = named[k[8:]].grad.cpu()
            if np.abs(v).max() < 1e-12:  # conv.0.bias ahead of the train-mode BN: mathematically zero
                assert torch.isfinite(a).all() and a.abs().max() < 1e-4 * np.abs(g["auxgrad/aux_head.conv.1.bias"]).max()
                continue
            assert rel_err(a, v) < 1e-3, (k, rel_err(a, v))


# ------------------------------------------------------------------------------------ 5. eval parity
def test_eval_skips_the_aux_head():
    from dformer_amd import kernels as K
    g = load("e2e_tiny_aux")
    rgb, dep, lab, bases = _inputs(g, 40)
    with_head, without = build(40), build(40, aux_rate=None)
    assert with_head.aux_head is not None and without.aux_head is None
    without.load_state_dict({k: v for k, v in with_head.state_dict().items() if not k.startswith("aux_head.")})
    for m in (with_head, without):
        m.decode_head.hamburger.ham.injected_bases = bases
        m.eval()
    with torch.no_grad():
        assert torch.equal(with_head(rgb, dep), without(rgb, dep))
    assert torch.equal(with_head.predict(rgb, dep), without.predict(rgb, dep))

    def tags(fn):
        K.ACCOUNT = []
        K.trace(1)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            K.trace(0)
            acct, K.ACCOUNT = K.ACCOUNT, None
        return [(a[-1], [K.kernel_name(f) for f in a[0]]) for a in acct]

    def evals():
        with torch.no_grad():
            with_head(rgb, dep)
        with_head.predict(rgb, dep)

    ev = tags(evals)
    assert len(ev) > 10 and not [t for t, _ in ev if t.startswith("aux")]
    assert not [n for _, names in ev for n in names if "_s1_kernel" in n]
    with_head.train()
    tr = tags(lambda: with_head(rgb, dep, lab)[0].backward())
    assert {t for t, _ in tr if t.startswith("aux")} == {"aux", "aux.bwd"}
    aux_kernels = [n for t, names in tr if t.startswith("aux") for n in names]
    assert any("im2col_s1_kernel" in n for n in aux_kernels) and any("col2im_s1_kernel" in n for n in aux_kernels)


# ------------------------------------------------------------------------------ 6. training plumbing
def test_aux_graphed_steps_match_eager_and_update_the_head():
    """Tiny 2 x 64x96, bf16, FusedAdamW: the aux parameters' flat gradient slots are written and the
    parameters move; two eager steps and two GraphedTrainStep replays agree bit for bit (the pattern of
    tests/test_graph_gpu.py::test_graphed_steps_match_eager)."""
    import bench
    from dformer_amd.segmentor import EncoderDecoder
    from dformer_amd.train import FusedAdamW, GraphedTrainStep, train_step
    dev = torch.device("cuda", 0)

    def make():
        cfg = bench.make_cfg("DFormer-Tiny", "ham")
        cfg["drop_path_rate"] = 0.0
        cfg["aux_rate"] = 0.4
        torch.manual_seed(3)
        m = EncoderDecoder(cfg=cfg)
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
    rgb, dep, lab = bench.synthetic_batch(2, 64, 96, cfg.num_classes, dev, 5)
    aux = dict(ma.aux_head.named_parameters())
    assert len(aux) == 6
    slots = {}
    for n, p in aux.items():
        grp = next(gr for gr in oa.groups if p in gr.slots)
        off, k = grp.slots[p]
        slots[n] = grp.grad[off:off + k]
        slots[n].fill_(float("nan"))
    before = {n: p.detach().clone() for n, p in aux.items()}
    la = [train_step(ma, oa, rgb, dep, lab).item()]
    for n, p in aux.items():
        assert torch.isfinite(slots[n]).all(), n          # the slot was written by this step's backward
        if n != "conv.0.bias":  # zero gradient ahead of the train-mode BN: rounding noise only
            assert slots[n].abs().max() > 0, n
            assert not torch.equal(p.detach(), before[n]), n
    la += [train_step(ma, oa, rgb, dep, lab).item() for _ in range(3)]
    g = GraphedTrainStep(mb, ob, rgb, dep, lab, warmup=2)
    lb = [g().item() for _ in range(2)]
    assert ob.step_count == oa.step_count == 4
    assert np.isfinite(la).all() and la[2:] == lb, (la, lb)
    for ga, gb_ in zip(oa.groups, ob.groups):
        assert torch.equal(ga.flat, gb_.flat) and torch.equal(ga.m, gb_.m) and torch.equal(ga.v, gb_.v)
