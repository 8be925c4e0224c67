"""The shared BatchNorm forward / backward (dformer_amd/batchnorm.py) under the decoders' conv + BN functions,
in eval mode (running statistics, a fixed per-channel affine in both directions) and in train mode, against
torch's own conv / linear / interpolate / batch_norm in fp32: the merged 1x1 function with and without a conv
bias, SqueezeFoldFn, and DecoderHead end to end. Outputs and every gradient at rel < 1e-4, the fp32 gate of
tests/test_aux_gpu.py::test_fcn_head_eval_vs_torch."""
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = [pytest.param(False, id="eval"), pytest.param(True, id="train")]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.manual_seed(0)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _randomise(bns, training):
    """Random affine and running statistics on every BN; returns the torch reference's own copies of the
    running statistics (F.batch_norm updates them in place in train mode)."""
    from dformer_amd.functional import invalidate_weights
    with torch.no_grad():
        for bn in bns:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-1, 1)
            bn.running_var.uniform_(0.5, 2)
            bn.train(training)
    invalidate_weights()
    return [(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns]


def _ref_bn(z, bn, run, training):
    return F.batch_norm(z, run[0], run[1], bn.weight, bn.bias, training, bn.momentum, bn.eps)


def _check_buffers(bns, before, ref_run, training):
    for bn, b0, r in zip(bns, before, ref_run):
        if training:  # updated like torch's
            assert rel(bn.running_mean, r[0]) < 1e-4 and rel(bn.running_var, r[1]) < 1e-4
            assert int(bn.num_batches_tracked) == 1
        else:  # bit-unchanged
            assert torch.equal(bn.running_mean, b0[0]) and torch.equal(bn.running_var, b0[1])
            assert int(bn.num_batches_tracked) == 0


def _check_grads(y, ref, leaves, ref_leaves, names, n_maps, zero=(), scale=None):
    """Every gradient of `y` against the reference's at rel < 1e-4; the first n_maps leaves are feature maps.
    `zero` names the biases ahead of a train-mode BN: their gradient is mathematically zero, so it is only
    bounded against the BN's beta gradient `scale` (the gate of
    tests/test_aux_gpu.py::test_fcn_head_fp32_vs_reference)."""
    dy = torch.randn_like(ref)
    g_ref = torch.autograd.grad(ref, ref_leaves, dy)
    g = torch.autograd.grad(y, leaves, dy)
    for i, (n, a, b) in enumerate(zip(names, g, g_ref)):
        if n in zero:
            bound = 1e-4 * dict(zip(names, g_ref))[scale].abs().max()
            print(f"{n}: |g| max {a.abs().max().item():.3e} (bound {bound.item():.3e})")
            assert torch.isfinite(a).all() and a.abs().max() < bound, n
            continue
        if i < n_maps:  # NHWC rows (or an NHWC map) against the reference's NCHW leaf
            b = b.permute(0, 2, 3, 1).reshape(a.shape)
        e = rel(a, b)
        print(f"{n}: rel {e:.3e}")
        assert e < 1e-4, (n, e)


# ------------------------------------------------------------------------------- 1. the merged 1x1 function
@pytest.mark.parametrize("training", MODES)
@pytest.mark.parametrize("form", ["res_relu", "plain", "bias_relu"])
def test_conv1_bn_act_vs_torch(form, training):
    """ConvModule.fused with a residual and ReLU, and with neither; and UPerHead._conv1, the form with a conv
    bias. Rows of a 2 x 3 x 5 map, 16 -> 24 channels."""
    from dformer_amd.decoders import ConvModule, UPerHead
    B, H, W, cin, cout = 2, 3, 5, 16, 24
    if form == "bias_relu":
        seq = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1), torch.nn.BatchNorm2d(cout),
                                  torch.nn.ReLU()).to(DEV)
        conv, bn = seq[0], seq[1]
    else:
        mod = ConvModule(cin, cout).to(DEV)
        conv, bn = mod.conv, mod.bn
    before = _randomise([bn], training)
    ref_run = [(m.clone(), v.clone()) for m, v in before]
    x = torch.randn(B * H * W, cin, device=DEV).requires_grad_()
    res = torch.randn(B * H * W, cout, device=DEV).requires_grad_() if form == "res_relu" else None
    if form == "bias_relu":
        y = UPerHead._conv1(types.SimpleNamespace(syncbn=False), seq, x)
    else:
        y = mod.fused(x, act=2 if form == "res_relu" else 0, res=res)

    def nchw(rows):
        return rows.detach().view(B, H, W, -1).permute(0, 3, 1, 2).contiguous().requires_grad_()

    x4 = nchw(x)
    ref = _ref_bn(F.conv2d(x4, conv.weight, conv.bias), bn, ref_run[0], training)
    leaves, ref_leaves, names = [x], [x4], ["x"]
    if res is not None:
        r4 = nchw(res)
        ref = ref + r4
        leaves, ref_leaves, names = leaves + [res], ref_leaves + [r4], names + ["res"]
    if form != "plain":
        ref = F.relu(ref)
    params = [conv.weight, bn.weight, bn.bias] + ([conv.bias] if conv.bias is not None else [])
    names += ["weight", "gamma", "beta"] + (["bias"] if conv.bias is not None else [])
    e = rel(y.view(B, H, W, cout).permute(0, 3, 1, 2), ref.detach())
    print(f"y: rel {e:.3e}")
    assert e < 1e-4
    _check_buffers([bn], before, ref_run, training)
    ref_rows = ref.permute(0, 2, 3, 1).reshape(B * H * W, cout)
    _check_grads(y, ref_rows, leaves + params, ref_leaves + params, names, len(leaves),
                 zero=("bias",) if training else (), scale="beta")


# ------------------------------------------------------------------------------------------ 2. SqueezeFoldFn
@pytest.mark.parametrize("training", MODES)
def test_squeeze_fold_vs_torch(training):
    """Three levels at (4, 6), (2, 3), (1, 2) with 8, 16, 24 channels into E = 16, B = 2, against resize + cat +
    1x1 conv + BN + ReLU (ham_head.py:226-234)."""
    from dformer_amd.decoders import ConvModule, SqueezeFoldFn
    B, E = 2, 16
    hw, chans = [(4, 6), (2, 3), (1, 2)], [8, 16, 24]
    sq = ConvModule(sum(chans), E, bn_eps=1e-3).to(DEV)
    before = _randomise([sq.bn], training)
    ref_run = [(m.clone(), v.clone()) for m, v in before]
    rows = [torch.randn(B * h * w, c, device=DEV).requires_grad_() for (h, w), c in zip(hw, chans)]
    y = SqueezeFoldFn.apply(B, hw, sq.bn, False, sq.conv.weight, sq.bn.weight, sq.bn.bias, *rows)
    maps = [r.detach().view(B, h, w, c).permute(0, 3, 1, 2).contiguous().requires_grad_()
            for r, (h, w), c in zip(rows, hw, chans)]
    cat = torch.cat([maps[0]] + [F.interpolate(m, hw[0], mode="bilinear", align_corners=False) for m in maps[1:]], 1)
    ref = F.relu(_ref_bn(F.conv2d(cat, sq.conv.weight), sq.bn, ref_run[0], training))
    ref_rows = ref.permute(0, 2, 3, 1).reshape(-1, E)
    e = rel(y, ref_rows.detach())
    print(f"y: rel {e:.3e}")
    assert e < 1e-4
    _check_buffers([sq.bn], before, ref_run, training)
    params = [sq.conv.weight, sq.bn.weight, sq.bn.bias]
    _check_grads(y, ref_rows, rows + params, maps + params, ["c0", "c1", "c2", "weight", "gamma", "beta"], 3)


# -------------------------------------------------------------------------------- 3. DecoderHead end to end
@pytest.mark.parametrize("training", MODES)
def test_decoder_head_vs_torch(training):
    """DecoderHead (MLPDecoder.py:22-81) with in_channels (8, 16, 24, 32), embed_dim 16, 5 classes, B = 2, maps
    at (8, 12) .. (1, 2); dropout inactive (eval mode, or ratio 0 in the train-mode case)."""
    from dformer_amd.decoders import DecoderHead
    B, E, ncls = 2, 16, 5
    hw, chans = [(8, 12), (4, 6), (2, 3), (1, 2)], (8, 16, 24, 32)
    head = DecoderHead(chans, ncls, embed_dim=E).to(DEV).train(training)
    head.dropout_ratio = 0.0
    fuse, bn = head.linear_fuse[0], head.linear_fuse[1]
    before = _randomise([bn], training)
    ref_run = [(m.clone(), v.clone()) for m, v in before]
    xs = [torch.randn(B, h, w, c, device=DEV).requires_grad_() for (h, w), c in zip(hw, chans)]
    y = head([x.permute(0, 3, 1, 2) for x in xs])
    assert tuple(y.shape) == (B, ncls) + hw[0]
    maps = [x.detach().permute(0, 3, 1, 2).contiguous().requires_grad_() for x in xs]
    ups = []
    for i, (m, (h, w)) in enumerate(zip(maps, hw)):
        lin = getattr(head, f"linear_c{i + 1}").proj
        t = F.linear(m.flatten(2).transpose(1, 2), lin.weight, lin.bias).permute(0, 2, 1).reshape(B, E, h, w)
        ups.append(t if i == 0 else F.interpolate(t, hw[0], mode="bilinear", align_corners=False))
    z = F.conv2d(torch.cat(ups[::-1], 1), fuse.weight, fuse.bias)  # cat order [c4 | c3 | c2 | c1]
    z = F.relu(_ref_bn(z, bn, ref_run[0], training))
    ref = F.conv2d(z, head.linear_pred.weight, head.linear_pred.bias)
    e = rel(y, ref.detach())
    print(f"logits: rel {e:.3e}")
    assert e < 1e-4
    _check_buffers([bn], before, ref_run, training)
    named = list(head.named_parameters())
    assert len(named) == 14
    names = [f"c{i + 1}" for i in range(4)] + [k for k, _ in named]
    params = [p for _, p in named]
    zero = [k for k in names if k.endswith("proj.bias") or k == "linear_fuse.0.bias"] if training else ()
    _check_grads(y, ref, xs + params, maps + params, names, 4, zero=zero, scale="linear_fuse.1.bias")
