"""The UPerNet decoder on the GPU (UPernet.py:8-146, builder.py:145-152): the implicit-GEMM 3x3 conv (forward,
input gradient, weight gradient) and the pyramid pooling against torch in fp64, UPerHead against the
reference's fp64 goldens (oracle/golden_decoders.py / golden_e2e.py), DFormer-Tiny + UPernet end to end, eval parity and the
optimizer / HIP-graph plumbing."""
import copy
import functools

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
# (B, H, W, Cin, Cout): minimal; single row + batch seam; Cin no multiple of 32 (every k-slice straddles taps);
# 5x7; several row tiles with image seams inside a tile and Cout no tile multiple; wgrad split-K across images;
# the bottleneck widths of DFormer-Tiny (2304 = 36 * 64) and DFormer-Large (2624 = 41 * 64) + UPernet
SHAPES = [(1, 1, 1, 8, 8), (2, 1, 5, 8, 40), (2, 3, 3, 40, 72), (2, 5, 7, 96, 40), (2, 9, 13, 64, 136),
          (3, 17, 23, 32, 16), (1, 2, 3, 2304, 16), (1, 2, 3, 2624, 16)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.manual_seed(0)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


def _rows(t4):
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


# ------------------------------------------------------------------ 1. the implicit-GEMM conv vs torch fp64
@functools.lru_cache(maxsize=None)
def _conv_case(shape, dt):
    """Operands rounded to dt, and F.conv2d with its three gradients in fp64 on the CPU, computed once per
    (shape, dtype) and shared by the conv tests: (x, w, b, dy) on the GPU, (y, gx, gw, gb) fp64 rows / tensors."""
    B, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    P = B * H * W
    x = torch.randn(P, cin, generator=g).to(dt)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).to(dt).float()  # exact in dt: the pack keeps it
    b = torch.randn(cout, generator=g)
    dy = torch.randn(P, cout, generator=g).to(dt)
    x4 = _nchw(x.double(), B, H, W).contiguous().requires_grad_()
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    y = F.conv2d(x4, w64, b64, padding=1)
    gx, gw, gb = torch.autograd.grad(y, [x4, w64, b64], _nchw(dy.double(), B, H, W))
    return (x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)), (_rows(y.detach()), _rows(gx), gw, gb)


def _slice_of_wider(t, fill):
    """t as a column slice (starting at column 8: still 16-byte aligned) of a wider buffer filled with `fill`."""
    buf = torch.full((t.shape[0], t.shape[1] + 24), fill, device=t.device, dtype=t.dtype)
    buf[:, 8:8 + t.shape[1]].copy_(t)
    return buf, buf[:, 8:8 + t.shape[1]]


def _untouched(buf, n, fill):
    return bool((buf[:, :8] == fill).all() and (buf[:, 8 + n:] == fill).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_conv_igemm_forward(shape, dt):
    from dformer_amd import kernels as K
    B, H, W, cin, cout = shape
    (x, w, b, _), (y_ref, _, _, _) = _conv_case(shape, dt)
    assert K.conv3_igemm_supported(dt, cin, cout)
    wp = K.conv3_weight_pack(w, dt, 9 * cin)
    y_nobias = y_ref - b.double().cpu()
    for wide in (False, True):
        xs = _slice_of_wider(x, 3.0)[1] if wide else x
        for bias, want in ((b, y_ref), (None, y_nobias)):
            if wide:
                ybuf, ys = _slice_of_wider(torch.zeros(B * H * W, cout, device=DEV, dtype=dt), 7.0)
                y = K.conv3_igemm(xs, (B, H, W), wp, bias, out=ys)
                assert _untouched(ybuf, cout, 7.0)
            else:
                y = K.conv3_igemm(xs, (B, H, W), wp, bias)
            assert y.dtype == dt and tuple(y.shape) == (B * H * W, cout)
            e = rel(y, want)
            print(f"fwd {shape} {dt} wide={wide} bias={bias is not None}: {e:.3e}")
            assert e < TOL[dt], (wide, bias is not None, e)
    if dt == torch.float32:  # the materialised path of the aux head on the same operands
        old = K.linear(K.conv3s1_im2col(x, (B, H, W)), wp, b)
        assert rel(K.conv3_igemm(x, (B, H, W), wp, b), old) < TOL[dt]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_conv_igemm_input_gradient(shape, dt):
    from dformer_amd import kernels as K
    B, H, W, cin, cout = shape
    (x, w, b, dy), (_, gx_ref, _, _) = _conv_case(shape, dt)
    wpt = K.conv3_weight_pack_dgrad(w, dt)
    assert tuple(wpt.shape) == (cin, 9 * cout)
    want_pack = K.conv3_weight_pack(w.permute(1, 0, 2, 3).flip(2, 3).contiguous(), dt, 9 * cout)
    assert torch.equal(wpt, want_pack)
    tol = TOL[dt] * (2 if dt != torch.float32 else 1)
    for wide in (False, True):
        dys = _slice_of_wider(dy, 5.0)[1] if wide else dy
        for accumulate in (False, True):
            g = torch.Generator().manual_seed(5)
            before = torch.randn(B * H * W, cin, generator=g).to(dt).to(DEV)
            if wide:
                buf, dx = _slice_of_wider(before, 9.0)
            else:
                buf, dx = None, before.clone()
            K.conv3_igemm(dys, (B, H, W), wpt, out=dx, accumulate=accumulate)
            want = gx_ref + (before.double().cpu() if accumulate else 0)
            e = rel(dx, want)
            print(f"dgrad {shape} {dt} wide={wide} acc={accumulate}: {e:.3e}")
            assert e < tol, (wide, accumulate, e)
            assert buf is None or _untouched(buf, cin, 9.0)
    if dt == torch.float32:
        old = K.conv3s1_col2im(K.linear_dgrad(dy, K.conv3_weight_pack(w, dt, 9 * cin)), (B, H, W), cin)
        assert rel(K.conv3_igemm(dy, (B, H, W), wpt), old) < TOL[dt]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_conv_igemm_weight_gradient(shape, dt):
    from dformer_amd import kernels as K
    B, H, W, cin, cout = shape
    (x, w, b, dy), (_, _, gw_ref, gb_ref) = _conv_case(shape, dt)
    tol = TOL[dt] * (2 if dt != torch.float32 else 1)
    for wide in (False, True):
        xs = _slice_of_wider(x, 3.0)[1] if wide else x
        dys = _slice_of_wider(dy, 5.0)[1] if wide else dy
        dwp, db = K.conv3_igemm_wgrad(dys, xs, (B, H, W), bias_grad=True)
        assert dwp.dtype == db.dtype == torch.float32 and tuple(dwp.shape) == (cout, 9 * cin)
        ew, eb = rel(K.conv3_weight_unpack(dwp, cin), gw_ref), rel(db, gb_ref)
        print(f"wgrad {shape} {dt} wide={wide}: dw {ew:.3e} db {eb:.3e}")
        assert ew < tol and eb < tol, (wide, ew, eb)
        dwp2, db2 = K.conv3_igemm_wgrad(dys, xs, (B, H, W), bias_grad=True)
        assert torch.equal(dwp, dwp2) and torch.equal(db, db2)  # fixed-order split-K: bit-identical
        assert rel(K.conv3_igemm_wgrad(dys, xs, (B, H, W)), dwp) < 1e-6  # without the ones column
    if dt == torch.float32:
        old = K.linear_wgrad(dy, K.conv3s1_im2col(x, (B, H, W)))
        assert rel(dwp, old) < TOL[dt]


def test_conv_igemm_wgrad_splits_across_images():
    """(3, 17, 23, 32, 16) is the split-K case: its workspace is not empty, and the seam between two splits
    lies inside the second image."""
    from dformer_amd import _lib
    need = _lib.lib.dfm_conv3s1_igemm_wgrad_workspace_size(_lib.BF16, 3, 17, 23, 32, 16, 1)
    assert need > 0 and (need // (16 * 296 * 4)) == 2 and 17 * 23 < 640 < 2 * 17 * 23


# ------------------------------------------------------------------------- 2. pyramid pooling vs torch fp64
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (15, 20), (17, 23)])
def test_ppm_pool(H, W, C, dt):
    from dformer_amd import kernels as K
    B, scales = 2, (1, 2, 3, 6)
    g = torch.Generator().manual_seed(H * 100 + W + C)
    x = torch.randn(B * H * W, C, generator=g).to(dt)
    x4 = _nchw(x.double(), B, H, W).contiguous().requires_grad_()
    refs = [F.adaptive_avg_pool2d(x4, s) for s in scales]
    y_ref = torch.cat([_rows(r.detach()) for r in refs], 0)
    dy = torch.randn(y_ref.shape, generator=g).to(dt)
    off, loss = 0, 0.0
    for s, r in zip(scales, refs):
        loss = loss + (r * _nchw(dy[off:off + B * s * s].double(), B, s, s)).sum()
        off += B * s * s
    gx_ref = _rows(torch.autograd.grad(loss, x4)[0])
    tol = TOL[dt] * (2 if dt != torch.float32 else 1)
    xbuf, xs = _slice_of_wider(x.to(DEV), 3.0)
    for src in (x.to(DEV), xs):
        y = K.ppm_pool(src, (B, H, W), scales)
        assert tuple(y.shape) == (B * 50, C) and y.dtype == dt
        assert rel(y, y_ref) < TOL[dt], rel(y, y_ref)
    for accumulate in (False, True):
        before = torch.randn(B * H * W, C, generator=g).to(dt).to(DEV)
        buf, dx = _slice_of_wider(before, 9.0)
        K.ppm_pool_bwd(dy.to(DEV), (B, H, W), scales, dx=dx, accumulate=accumulate)
        want = gx_ref + (before.double().cpu() if accumulate else 0)
        assert rel(dx, want) < tol, (accumulate, rel(dx, want))
        assert _untouched(buf, C, 9.0)
        dx2 = before.clone()
        K.ppm_pool_bwd(dy.to(DEV), (B, H, W), scales, dx=dx2, accumulate=accumulate)
        assert torch.equal(dx2, dx)  # one owner per element, fixed order
    assert rel(K.ppm_pool(x.to(DEV), (B, H, W), (2,)), _rows(refs[1].detach())) < TOL[dt]  # fewer scales


# ------------------------------------------------------------------------ 3. UPerHead vs the reference
PRE_BN_BIASES = ([f"psp_modules.{i}.1.bias" for i in range(4)] + ["bottleneck.0.bias", "fpn_bottleneck.0.bias"] +
                 [f"lateral_convs.{i}.0.bias" for i in range(3)] + [f"fpn_convs.{i}.0.bias" for i in range(3)])


def _bn_bias_of(k):
    head, idx, _ = k.rsplit(".", 2)
    return f"{head}.{int(idx) + 1}.bias"


def _uper_head(g):
    from dformer_amd.decoders import UPerHead
    from dformer_amd.functional import invalidate_weights
    B, channels, seed = [int(v) for v in g["meta"]]
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    head = UPerHead([s[0] for s in shapes], num_classes=40, channels=channels)
    sd = head.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    invalidate_weights()
    return head.cuda().train(), B, shapes, seed


def _head_inputs(name, seed, B, shapes, dt=torch.float32, grad=True):
    leaves = []
    for i, (c, h, w) in enumerate(shapes):
        a = torch.from_numpy(gen.normal(f"{name}#{seed}/x{i}", (B, c, h, w))).float().cuda()
        leaves.append(a.permute(0, 2, 3, 1).contiguous().to(dt).requires_grad_(grad))
    return leaves


@pytest.mark.parametrize("name", ["uperhead_c32", "uperhead_c64"])
def test_uper_head_fp32_vs_reference(name):
    g = load(name)
    head, B, shapes, seed = _uper_head(g)
    leaves = _head_inputs(name, seed, B, shapes)
    y = head([l.permute(0, 3, 1, 2) for l in leaves])
    assert tuple(y.shape) == (B, 40) + shapes[0][1:]
    y.backward(torch.from_numpy(gen.normal(f"{name}#{seed}/gy", tuple(y.shape))).float().cuda())
    e = rel_err(y.detach().cpu(), g["y"])
    print(f"{name}: y {e:.3e}")
    assert e < 1e-4
    for i, l in enumerate(leaves):
        ei = rel_err(l.grad.permute(0, 3, 1, 2).cpu(), g[f"gx/{i}"])
        print(f"{name}: gx/{i} {ei:.3e}")
        assert ei < 1e-3, (i, ei)
    grads = {k: p.grad.cpu() for k, p in head.named_parameters()}
    # a conv bias ahead of a train-mode BN: its gradient is mathematically zero (the reference gives ~1e-15),
    # so it is out of the relative gates and bounded against the BN bias's gradient, as for the aux head
    gated = {k: v for k, v in g.items() if k[5:] not in PRE_BN_BIASES}
    assert len([k for k in g if k.startswith(("grad/", "gradfp/"))]) == len(grads) == 50
    worst = check_param_grads(gated, grads, 1e-3, atol=1e-6)
    print(f"{name}: worst parameter gradient {worst:.3e}")
    for k in PRE_BN_BIASES:
        b0 = grads[k]
        assert torch.isfinite(b0).all() and b0.abs().max() < 1e-4 * np.abs(g["grad/" + _bn_bias_of(k)]).max(), k
    bufs = dict(head.named_buffers())
    nbuf = 0
    for k, v in g.items():
        if k.startswith("buf/"):
            nbuf += 1
            assert rel_err(bufs[k[4:]].cpu(), v) < 1e-4, k
    assert nbuf == 24 and int(bufs["fpn_bottleneck.1.num_batches_tracked"]) == 1


@pytest.mark.parametrize("dt,key", [(torch.bfloat16, "env_bf16/y"), (torch.float16, "env_f16/y")])
@pytest.mark.parametrize("name", ["uperhead_c32", "uperhead_c64"])
def test_uper_head_16bit_vs_reference_envelope(name, dt, key):
    """Output within 1.5 x the reference's own autocast error on the same input, floored at the conv gate."""
    g = load(name)
    head, B, shapes, seed = _uper_head(g)
    leaves = _head_inputs(name, seed, B, shapes, dt, grad=False)
    with torch.no_grad():
        y = head([l.permute(0, 3, 1, 2) for l in leaves])
    assert y.dtype == dt
    e = rel_err(y.float().cpu(), g["y"])
    print(f"{name} {dt}: {e:.3e} (reference envelope {float(g[key]):.3e})")
    assert e <= max(1.5 * float(g[key]), TOL[dt]), (e, float(g[key]))


def _torch_uper_forward(head, xs):
    """UPerHead's graph in plain torch on the module's own (copied) submodules: the out-of-place top-down sum."""
    lat = [seq(x) for seq, x in zip(head.lateral_convs, xs)]
    x = xs[-1]
    psp = [x] + [F.interpolate(seq(x), size=x.shape[2:], mode="bilinear", align_corners=False)
                 for seq in head.psp_modules]
    lat.append(head.bottleneck(torch.cat(psp, 1)))
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="bilinear", align_corners=False)
    outs = [head.fpn_convs[i](lat[i]) for i in range(len(lat) - 1)] + [lat[-1]]
    outs = [outs[0]] + [F.interpolate(o, size=outs[0].shape[2:], mode="bilinear", align_corners=False)
                        for o in outs[1:]]
    return head.conv_seg(head.fpn_bottleneck(torch.cat(outs, 1)))


@pytest.mark.parametrize("in_ch,channels,sizes", [([16, 32, 64, 96], 32, [(9, 13), (5, 7), (3, 4), (2, 2)]),
                                                  ([32, 64, 128, 256], 64, [(12, 20), (6, 10), (3, 5), (2, 3)])])
def test_uper_head_eval_vs_torch(in_ch, channels, sizes):
    """Eval mode: running statistics as a fixed affine (untouched) and the conv biases, against the same module
    in torch fp32 on the CPU. Output 1e-4; input gradients 1e-3, the train-mode gradient gate."""
    from dformer_amd.decoders import UPerHead
    from dformer_amd.functional import invalidate_weights
    torch.manual_seed(1)
    head = UPerHead(in_ch, channels=channels)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
                m.running_mean.uniform_(-0.5, 0.5)
                m.running_var.uniform_(0.5, 2)
            if isinstance(m, torch.nn.Conv2d):
                m.bias.uniform_(-0.5, 0.5)
    ref_head = copy.deepcopy(head).eval()
    head = head.cuda().eval()
    invalidate_weights()
    B = 2
    xs = [torch.randn(B, c, h, w, requires_grad=True) for c, (h, w) in zip(in_ch, sizes)]
    ref = _torch_uper_forward(ref_head, xs)
    dy = torch.randn_like(ref)
    g_ref = torch.autograd.grad(ref, xs, dy)
    leaves = [x.detach().cuda().permute(0, 2, 3, 1).contiguous().requires_grad_() for x in xs]
    y = head([l.permute(0, 3, 1, 2) for l in leaves])
    assert rel(y, ref.detach()) < 1e-4, rel(y, ref.detach())
    sd, rsd = head.state_dict(), ref_head.state_dict()
    for k in sd:
        if "running" in k or "num_batches" in k:
            assert torch.equal(sd[k].cpu(), rsd[k]), k
    gx = torch.autograd.grad(y, leaves, dy.cuda())
    for a, b in zip(gx, g_ref):
        assert rel(a.permute(0, 3, 1, 2), b) < 1e-3, rel(a.permute(0, 3, 1, 2), b)


# ------------------------------------------------------------------------------------ 4. end to end
def build(**extra):
    from dformer_amd.segmentor import EncoderDecoder
    cfg = Cfg(backbone="DFormer-Tiny", decoder="UPernet", decoder_embed_dim=512, num_classes=40, drop_path_rate=0.0,
              bn_eps=1e-3, bn_momentum=0.1, background=255, **extra)
    model = EncoderDecoder(cfg=cfg, syncbn=False)
    sd = model.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    return model.cuda()


def _inputs(g):
    B, H, W, ncls, seed = [int(v) for v in g["meta"]]
    rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=seed)
    return (torch.from_numpy(rgb_np).float().cuda(), torch.from_numpy(dep_np).float().cuda(),
            torch.from_numpy(gen.labels(B, H, W, ncls)).cuda())


def test_upernet_training_forward_fp32_vs_reference():
    """`low` / `aux_low` 1e-4, loss 1e-5, every gradient fingerprint within max(1e-4, 10 x env), the fp32_gate of
    tests/test_segmentor_gpu.py. The golden has no no-flip guarantee at 512 channels (its ReLU margin is recorded
    in the file): the gradients are gated through the reference's own fp32 envelope only."""
    g = load("e2e_tiny_uper")
    rgb, dep, lab = _inputs(g)
    model = build().train()
    seen = {}
    head_forward = model.decode_head.forward  # the segmentor calls .forward itself: no module hook fires

    def keep_low(outs):
        seen["low"] = head_forward(outs)
        return seen["low"]

    model.decode_head.forward = keep_low
    model.aux_head.register_forward_hook(lambda m, a, o: seen.__setitem__("aux_low", o.detach()))
    loss, out = model(rgb, dep, lab)
    loss.backward()
    torch.cuda.synchronize()
    assert tuple(seen["low"].shape) == tuple(g["low"].shape) == (2, 40, 16, 24)  # the main head is at x4
    assert tuple(seen["aux_low"].shape) == tuple(g["aux_low"].shape) == (2, 40, 4, 6)
    assert tuple(out.shape) == (2, 40, 64, 96)
    el, ea = rel_err(seen["low"].detach().float().cpu(), g["low"]),rel_err(seen["aux_low"].float().cpu(), g["aux_low"])
    print(f"low {el:.3e} aux_low {ea:.3e} loss {loss.item():.7f} vs {float(g['loss']):.7f}")
    assert el < 1e-4 and ea < 1e-4
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    assert abs(float(g["loss"]) - (float(g["loss_main"]) + 0.4 * float(g["loss_aux"]))) < 1e-12
    named = dict(model.named_parameters())
    bad, seen_fp = [], 0
    for k, v in g.items():
        if k.startswith("gfp/"):
            seen_fp += 1
            e = fp_rel_err(gen.fingerprint(named[k[4:]].grad.cpu().double().numpy(), 16), v, atol=1e-4)
            if e > max(1e-4, 10.0 * float(g["env/" + k])):
                bad.append((k, e, float(g["env/" + k])))
    print(f"{seen_fp} gradient fingerprints, {len(bad)} outside the gate: {bad[:10]}")
    assert seen_fp > 200 and not bad, bad[:10]


# ----------------------------------------------------------------------------- 5. eval and training plumbing
def test_upernet_eval_paths_and_aux_head_is_skipped():
    from dformer_amd import kernels as K
    g = load("e2e_tiny_uper")
    rgb, dep, lab = _inputs(g)
    model = build().eval()
    with torch.no_grad():
        out = model(rgb, dep)
    pred = model.predict(rgb, dep)
    assert tuple(out.shape) == (2, 40, 64, 96) and tuple(pred.shape) == (2, 64, 96)
    # predict is forward(...).argmax(1): a pixel may differ only inside the near-tie band of
    # tests/test_predict_gpu.py (fp32 interpolation of four taps errs by a few 1e-7 of their magnitude)
    top = out.double().topk(2, dim=1).values
    diff = pred.long() != out.argmax(1)
    assert bool(((top[:, 0] - top[:, 1])[diff] <= 1e-5 * out.abs().max().double()).all()), int(diff.sum())
    assert int(diff.sum()) <= 1e-3 * diff.numel()

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
            model(rgb, dep)
        model.predict(rgb, dep)

    ev = tags(evals)
    assert len(ev) > 10 and not [t for t, _ in ev if t.startswith("aux")]
    assert not [n for _, names in ev for n in names if "_s1_kernel" in n]  # the aux head's gather
    assert any("conv3_igemm_fwd_kernel" in n for _, names in ev for n in names)
    model.train()
    tr = tags(lambda: model(rgb, dep, lab)[0].backward())
    assert {t for t, _ in tr if t.startswith("aux")} == {"aux", "aux.bwd"}
    dec = [n for t, names in tr if t.startswith("decoder") for n in names]
    for kern in ("conv3_igemm_fwd_kernel", "conv3_igemm_wgrad_kernel", "ppm_pool_fwd_kernel", "ppm_pool_bwd_kernel"):
        assert any(kern in n for n in dec), kern
    assert not any("_s1_kernel" in n for n in dec)  # nothing of size P x 9*Cin in the main head


def test_upernet_graphed_steps_match_eager_and_update_both_heads():
    """Tiny 2 x 64x96, bf16, FusedAdamW: every decode_head / aux_head parameter's flat gradient slot is written
    and the parameters move; two eager steps and two GraphedTrainStep replays agree bit for bit (the pattern
    of tests/test_aux_gpu.py::test_aux_graphed_steps_match_eager_and_update_the_head)."""
    import bench
    from dformer_amd.segmentor import EncoderDecoder
    from dformer_amd.train import FusedAdamW, GraphedTrainStep, train_step
    dev = torch.device("cuda", 0)

    def make():
        cfg = bench.make_cfg("DFormer-Tiny", "UPernet")
        cfg["drop_path_rate"] = 0.0
        torch.manual_seed(3)
        m = EncoderDecoder(cfg=cfg).to(dev).set_compute_dtype(torch.bfloat16)
        m.return_logits = False
        return cfg, m.train()

    (cfg, ma), (_, mb) = make(), make()
    oa = FusedAdamW(ma, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
    ob = FusedAdamW(mb, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
    rgb, dep, lab = bench.synthetic_batch(2, 64, 96, cfg.num_classes, dev, 5)
    heads = {n: p for n, p in ma.named_parameters() if n.startswith(("decode_head.", "aux_head."))}
    assert len(heads) == 50 + 6
    pre_bn = {"decode_head." + k for k in PRE_BN_BIASES} | {"aux_head.conv.0.bias"}
    slots = {}
    for n, p in heads.items():
        grp = next(gr for gr in oa.groups if p in gr.slots)
        off, k = grp.slots[p]
        slots[n] = grp.grad[off:off + k]
        slots[n].fill_(float("nan"))
    before = {n: p.detach().clone() for n, p in heads.items()}
    la = [train_step(ma, oa, rgb, dep, lab).item()]
    for n, p in heads.items():
        assert torch.isfinite(slots[n]).all(), n          # the slot was written by this step's backward
        if n not in pre_bn:  # zero gradient ahead of a train-mode BN: rounding noise only
            assert slots[n].abs().max() > 0, n
            assert not torch.equal(p.detach(), before[n]), n
    la += [train_step(ma, oa, rgb, dep, lab).item() for _ in range(3)]
    g = GraphedTrainStep(mb, ob, rgb, dep, lab, warmup=2)
    lb = [g().item() for _ in range(2)]
    assert ob.step_count == oa.step_count == 4
    assert np.isfinite(la).all() and la[2:] == lb, (la, lb)
    for ga, gb_ in zip(oa.groups, ob.groups):
        assert torch.equal(ga.flat, gb_.flat) and torch.equal(ga.m, gb_.m) and torch.equal(ga.v, gb_.v)
