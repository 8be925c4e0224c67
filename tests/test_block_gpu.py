"""Parity of the HIP encoder Block against the reference goldens (fp32, 1e-3) and the oracle (bf16)."""
import json
import os

import numpy as np
import pytest
import torch

import dformer_ref as R
import gen
from goldens import MODELS, RATIOS, check_param_grads, load, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ["block_tiny_s0", "block_tiny_s1", "block_tiny_s3_last", "block_base_s0", "block_base_s1",
          "block_base_s2", "block_base_s3", "block_base_s3_last", "block_large_s1", "block_large_s2",
          "block_droppath_base_s1", "block_tiny_s3_last_ye", "block_base_s0_120x160"]


def make_block(name, device="cpu"):
    from dformer_amd.encoder import Block
    g = load(name)
    B, H, W, C, stage, last, dp = [int(v) for v in g["meta"]]
    model = "base" if "droppath" in name else name.split("_")[1]
    m = MODELS[model]
    depth = m["depths"][stage]
    j = depth - 1 if last else 0
    blk = Block(index=0, dim=C, num_head=m["heads"][stage], mlp_ratio=RATIOS[stage], block_index=depth - j,
                window=0 if stage == 0 else 7, dropout_layer=dict(type="DropPath", drop_prob=dp / 1e6),
                drop_depth=bool(last))
    sd = blk.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()])
    blk.load_state_dict({k: torch.from_numpy(np.asarray(v)).float() for k, v in vals.items()})
    return g, blk.to(device), (B, H, W, C, stage, bool(last), dp / 1e6)


@pytest.mark.parametrize("name", BLOCKS)
def test_block_state_dict_matches_reference_layout(name):
    g, blk, (B, H, W, C, stage, last, dp) = make_block(name)
    shapes = R.block_shapes(C, RATIOS[stage], 0 if stage == 0 else 7, last)
    sd = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    assert sd == shapes
    names = {k.split("/", 1)[1] for k in g if k.startswith("grad")}
    assert names <= set(sd)


def run_block(name, dtype):
    from dformer_amd.functional import invalidate_weights
    g, blk, (B, H, W, C, stage, last, dp) = make_block(name, "cuda")
    invalidate_weights()
    blk.train()
    if dp:
        blk.drop_path_masks = [torch.tensor(m) for m in ([1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 1.0])]
    x = torch.from_numpy(gen.normal(name + "/x", (B, H, W, C))).to("cuda", dtype).requires_grad_()
    xe = torch.from_numpy(gen.normal(name + "/xe", (B, H, W, C // 2))).to("cuda", dtype).requires_grad_()
    y, ye = blk(x, xe)
    gy = torch.from_numpy(gen.normal(name + "/gy", y.shape)).to("cuda", dtype)
    if "y_e" not in g:  # a drop_depth Block whose x_e output the golden's loss leaves out
        y.backward(gy)
    else:  # every other Block, and a drop_depth Block's e_back output (DFormer.py:133, 177-181; *_ye)
        gye = torch.from_numpy(gen.normal(name + "/gye", ye.shape)).to("cuda", dtype)
        torch.autograd.backward([y, ye], [gy, gye])
    torch.cuda.synchronize()
    return g, blk, x, xe, y, ye, "y_e" not in g


@pytest.mark.gpu
@pytest.mark.parametrize("name", BLOCKS)
def test_block_fp32_vs_reference_goldens(name):
    fp32_golden_check(*run_block(name, torch.float32))


def fp32_golden_check(g, blk, x, xe, y, ye, last):
    tol = 1e-3
    assert rel_err(y.cpu(), g["y"]) < tol
    assert rel_err(x.grad.cpu(), g["gx"]) < tol
    if not last:
        assert rel_err(ye.cpu(), g["y_e"]) < tol
        assert rel_err(xe.grad.cpu(), g["gxe"]) < tol
    grads = {k: p.grad.cpu() for k, p in blk.named_parameters() if p.grad is not None}
    check_param_grads(g, grads, tol)


# bf16 gates relative to the reference's OWN bf16 error on the same Block (tests/golden/bf16env_block_*,
# oracle/golden_blocks.py golden_block_bf16_env: reference float32 under torch.autocast(bfloat16) vs
# its fp64 golden, per output and per parameter gradient). The HIP path stores every activation in
# bf16 (autocast keeps LN / GELU / elementwise results in fp32), so each error may be up to
# BF16_ENV_MULT times the envelope, the envelope floored at one bf16 rounding (2^-8): gates that
# move with what bf16 can do on that tensor instead of one flat number.
BF16_ENV_MULT = 4.0
BF16_FLOOR = 2.0 ** -8


BF16_BLOCKS = ["block_tiny_s1", "block_base_s0", "block_base_s1", "block_base_s2", "block_base_s3",
               "block_base_s3_last", "block_large_s2", "block_base_s0_120x160"]
# ConvFFN routes (functional.FUSED_FFN): the op-level chain, the fused forward + op-level backward, fused
# forward + fused backward, each forced onto every Block (plane threshold 0) so the small golden planes take
# the fused kernels too; and the default "auto" (fused forward on planes of >= FUSED_FWD_MIN_PLANE pixels)
# on the 480x640 stage-0 plane, the route the bench runs
FFN_CASES = [(n, m) for n in BF16_BLOCKS for m in (False, "fwd", True)] + [("block_base_s0_120x160", "auto")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ffn", FFN_CASES)
def test_block_bf16_vs_reference_goldens(name, ffn, monkeypatch):
    """bf16 per Block: forward also within 1e-2 rel-to-max; forward, input gradients and
    EVERY parameter gradient within BF16_ENV_MULT x the reference's own bf16 envelope, on every ConvFFN
    route; the fused kernels must actually run where the route and the shape select them."""
    from dformer_amd import functional as Fn, kernels as Kk
    monkeypatch.setattr(Fn, "FUSED_FFN", ffn)
    if ffn != "auto":
        monkeypatch.setattr(Fn, "FUSED_FWD_MIN_PLANE", 0)
    calls = {"fwd": 0, "bwd": 0}
    for which in ("fwd", "bwd"):
        orig = getattr(Kk, "convffn_" + which)

        def counted(*a, _o=orig, _w=which, **k):
            calls[_w] += 1
            return _o(*a, **k)
        monkeypatch.setattr(Kk, "convffn_" + which, counted)
    g, blk, x, xe, y, ye, last = run_block(name, torch.bfloat16)
    B, H, W, C, stage = [int(v) for v in g["meta"][:5]]
    supported = any(Kk.convffn_supported(torch.bfloat16, (B, H, W), c, RATIOS[stage] * c)
                    for c in ((C,) if last else (C, C // 2)))
    fused_fwd = supported and (ffn in ("fwd", True) or (ffn == "auto" and H * W >= Fn.FUSED_FWD_MIN_PLANE))
    assert (calls["fwd"] > 0) == fused_fwd, (calls, supported)
    assert (calls["bwd"] > 0) == (supported and ffn is True), (calls, supported)
    grads = {k: p.grad for k, p in blk.named_parameters() if p.grad is not None}
    bf16_envelope_check(name, f"ffn-{ffn}", g, y, ye, x.grad, xe.grad, grads, last)


def bf16_envelope_check(name, tag, g, y, ye, gx, gxe, grads, last):
    """Gate one bf16 Block's outputs / input gradients / parameter gradients against the reference golden at
    BF16_ENV_MULT x the reference's own bf16 error (bf16env_<name>), floored at one bf16 rounding."""
    from goldens import fp_rel_err
    env = load("bf16env_" + name)

    def gate(key):
        return BF16_ENV_MULT * max(float(env["env/" + key]), BF16_FLOOR)

    errs = {"y": rel_err(y.float().cpu(), g["y"]), "gx": rel_err(gx.float().cpu(), g["gx"])}
    if not last:
        errs["y_e"] = rel_err(ye.float().cpu(), g["y_e"])
        errs["gxe"] = rel_err(gxe.float().cpu(), g["gxe"])
    assert errs["y"] < 1e-2 and errs.get("y_e", 0.0) < 1e-2, errs
    for k in env:
        if k.startswith("env/grad/"):
            n = k[len("env/grad/"):]
            a = grads[n].detach().double().cpu()
            if "grad/" + n in g:
                errs["grad/" + n] = rel_err(a, g["grad/" + n])
            else:
                errs["grad/" + n] = fp_rel_err(gen.fingerprint(a.numpy(), 256), g["gradfp/" + n])
    ratios = {k: v / max(float(env["env/" + k]), BF16_FLOOR) for k, v in errs.items()}
    worst = max(ratios, key=ratios.get)
    print(f"{name} {tag}: worst {worst} err {errs[worst]:.3e} = {ratios[worst]:.2f} x envelope")
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):  # the measured ratios, for DESIGN.md (GPU box runs only)
        with open(os.path.join(out, f"bf16env_ratios_{name}_{tag}.json"), "w") as fh:
            json.dump({"errs": errs, "ratios": ratios, "mult": BF16_ENV_MULT, "floor": BF16_FLOOR}, fh, indent=1)
    bad = {k: (errs[k], gate(k)) for k in errs if errs[k] >= gate(k)}
    assert not bad, bad


WG_STREAM_BLOCKS = ["block_base_s2",       # 2x9x10x256, window 7: pooled branch and both ConvFFN forks
                    "block_base_s0",       # 1x16x20x64, window 0
                    "block_base_s3_last"]  # drop_depth: no ConvFFN fork


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", WG_STREAM_BLOCKS)
def test_block_wgrad_stream_bit_equal(name, dtype, monkeypatch):
    """Every weight-gradient group of the Block's backward on the weight-gradient stream
    (kernels.WG_STREAM_MIN_FLOPS = 0; the goldens' groups are all below the default threshold) against none
    there (inf): outputs, input gradients and every parameter gradient bit-equal, the stream used exactly in
    the first run, and the first run within the golden gates of the tests above."""
    from dformer_amd import kernels as Kk, streams
    launched_on = []
    check = Kk.check

    def logged(status, what):
        launched_on.append(torch.cuda.current_stream().cuda_stream)
        return check(status, what)
    monkeypatch.setattr(Kk, "check", logged)
    runs = []
    for min_flops in (0, float("inf")):
        monkeypatch.setattr(Kk, "WG_STREAM_MIN_FLOPS", min_flops)
        del launched_on[:]
        g, blk, x, xe, y, ye, last = run = run_block(name, dtype)
        wg = streams.side_stream(x.device, "wgrad").cuda_stream
        assert (launched_on.count(wg) > 0) == (min_flops == 0), (min_flops, launched_on.count(wg), len(launched_on))
        runs.append(run)
    (g, blk0, x0, xe0, y0, ye0, last), (_, blk1, x1, xe1, y1, ye1, _) = runs
    assert torch.equal(y0, y1) and torch.equal(ye0, ye1)
    assert torch.equal(x0.grad, x1.grad) and torch.equal(xe0.grad, xe1.grad)
    g0 = {k: p.grad for k, p in blk0.named_parameters() if p.grad is not None}
    g1 = {k: p.grad for k, p in blk1.named_parameters() if p.grad is not None}
    assert g0.keys() == g1.keys() and len(g0) > 0
    differ = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not differ, differ
    if dtype == torch.float32:
        fp32_golden_check(*runs[0])
    else:
        bf16_envelope_check(name, "wgstream", g, y0, ye0, x0.grad, xe0.grad, g0, last)
