"""The folded memory passes of the Block backward (functional.FOLD_BWD_PASSES): the residual backward with
several rows in flight and its two-problem launch, the GELU' scale inside the 7x7 input gradient, the depth
branch's pooled-query gradient inside the LayerNorm backward, and the two forward pools in one launch.

The residual kernel is checked against a float64 reference at test_kernels_gpu.py's bounds; every fold is
checked for BIT equality with the unfolded pair of calls it replaces, and the Block for bit equality between
FOLD_BWD_PASSES True and False. The C-ABI Block is compared with the unfolded Python route at
test_block_capi_gpu.py's tolerances: the two routes group their GEMMs differently (see that file), so they
were never bit-equal to each other."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # tests/test_kernels_gpu.py


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


def rnd(*shape, dt=torch.float32, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, device=DEV, generator=g).to(dt)


def col_slice(t, pad=8):
    """t's values as a column slice of a wider buffer (leading dimension different from the width)."""
    wide = torch.full((t.shape[0], t.shape[1] + 2 * pad), 7.0, device=t.device, dtype=t.dtype)
    wide[:, pad:pad + t.shape[1]] = t
    return wide[:, pad:pad + t.shape[1]]


# ------------------------------------------------------------------------------- A: residual_bwd
RES_BLOCKS, RES_UNROLL = 512, 4  # elementwise.hip


def thread_rows(rows, C):
    """Row counts of the kernel's threads: the launch geometry of dfm_residual_bwd restated."""
    nblk = min(RES_BLOCKS, max(1, rows // 64))
    per = -(-rows // nblk)
    RL = 256 // (C // 8)
    out = set()
    for b in (0, nblk - 1):
        r0, r1 = b * per, min(rows, b * per + per)
        out |= {-(-(r1 - r0 - rl) // RL) for rl in range(RL) if r1 - r0 - rl > 0}
    return out, per, RL


def rows_for(C, n):
    """A row count that leaves some thread exactly n rows (one block where that fits, else all 512)."""
    RL = 256 // (C // 8)
    return RL * n if RL * n < 128 else RES_BLOCKS * RL * n - 3


RES_CASES = [(C, rows) for C in (8, 48, 256, 2048) for rows in
             sorted({1, 63, 64 * 3 + 5} | {rows_for(C, n) for n in (1, 2, 3, 5)})]


def test_residual_cases_reach_the_unroll_tail():
    for C in (8, 48, 256, 2048):
        for n in (1, 2, 3, 5):
            assert n in thread_rows(rows_for(C, n), C)[0], (C, n)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("scales", ["both", "none", "one_image", "sliced"])
@pytest.mark.parametrize("C,rows", RES_CASES)
def test_residual_bwd_vs_float64(C, rows, scales, dt):
    k = K()
    counts, per, RL = thread_rows(rows, C)
    dout, f = rnd(rows, C, dt=dt, seed=1), rnd(rows, C, dt=dt, seed=2)
    ls = rs = None
    rps = 1
    if scales != "none":
        ls = torch.rand(C, device=DEV) + 0.5
        # rows per scale: one image, or a count dividing neither a block's rows nor a thread's unrolled group
        rps = rows if scales == "one_image" else next(p for p in (7, 11, 13, 17)
                                                       if per % p and (RES_UNROLL * RL) % p)
        rs = torch.rand(-(-rows // rps), device=DEV)
    df = None
    if scales == "sliced":
        dout, f = col_slice(dout), col_slice(f)
        df = col_slice(torch.zeros(rows, C, device=DEV, dtype=dt))
    df, dls = k.residual_bwd(dout, f, ls, rs, rps, df=df)
    rsx = 1.0 if rs is None else rs.double().repeat_interleave(rps)[:rows, None]
    lsx = 1.0 if ls is None else ls.double()
    err_df = rel(df, dout.double() * lsx * rsx)
    err_dls = rel(dls, (dout.double() * f.double() * rsx).sum(0))
    print(f"residual_bwd C={C} rows={rows} {scales} {dt}: thread rows {sorted(counts)} df {err_df:.2e} dls {err_dls:.2e}")
    assert err_df < TOL[dt]
    assert err_dls < TOL[dt]
    if scales == "sliced":  # nothing outside the slice was written
        base = df._base if df._base is not None else df
        assert (base[:, :8] == 7).all() and (base[:, -8:] == 7).all()


# ------------------------------------------------------------------------------- B: residual_bwd2
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("rps", [(100, 100), (50, 200)])
@pytest.mark.parametrize("deferred", [False, True])
def test_residual_bwd2_bit_equal_to_two_calls(dt, rps, deferred):
    k = K()
    rows, C1, C2 = 200, 32, 16
    d1, f1, d2, f2 = (rnd(rows, c, dt=dt, seed=s) for s, c in ((1, C1), (2, C1), (3, C2), (4, C2)))
    ls1, ls2 = torch.rand(C1, device=DEV), torch.rand(C2, device=DEV)
    rs1, rs2 = torch.rand(rows // rps[0], device=DEV), torch.rand(rows // rps[1], device=DEV)
    rs1[0] = 0.0  # a dropped sample
    ref = torch.zeros(rows, C1 + C2, device=DEV, dtype=dt)
    got = torch.zeros_like(ref)

    def pair():
        _, a = k.residual_bwd(d1, f1, ls1, rs1, rps[0], df=ref[:, :C1])
        _, b = k.residual_bwd(d2, f2, ls2, rs2, rps[1], df=ref[:, C1:])
        return a, b

    def one():
        return k.residual_bwd2(d1, f1, ls1, rs1, rps[0], got[:, :C1], d2, f2, ls2, rs2, rps[1], got[:, C1:])

    if deferred:  # second stages described to the group and summed at its end
        with k.wgrad_group():
            a, b = pair()
        with k.wgrad_group():
            a2, b2 = one()
    else:
        (a, b), (a2, b2) = pair(), one()
    torch.cuda.synchronize()
    assert torch.equal(ref, got)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    assert torch.isfinite(a2).all() and torch.isfinite(b2).all()


# ------------------------------------------------------------------------------- C: dwconv_bwd_data_mul
DW_PLANES = [(5, 6), (11, 13), (30, 40)]


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("C", [8, 24, 64, 256])
@pytest.mark.parametrize("plane", DW_PLANES)
@pytest.mark.parametrize("acc", [False, True])
def test_dwconv_bwd_data_mul_bit_equal_to_pair(plane, C, k, acc, dt):
    kk = K()
    B, (H, W) = 2, plane
    P = B * H * W
    dy, mul = rnd(P, C, dt=dt, seed=1), rnd(P, C, dt=dt, seed=2)
    w = rnd(C, 1, k, k, seed=3) / k
    prior = rnd(P, C, dt=dt, seed=4) if acc else None  # another tensor than dx
    dg = prior.clone() if acc else torch.empty(P, C, device=DEV, dtype=dt)
    kk.dwconv_bwd_data(dy, (B, H, W), w, k, dx=dg, accumulate=acc)
    ref = kk.scale_mul(dg, mul=mul)
    out = col_slice(torch.zeros(P, C, device=DEV, dtype=dt))  # ld != C
    got = kk.dwconv_bwd_data_mul(dy, (B, H, W), w, k, mul, prior=prior, dx=out)
    torch.cuda.synchronize()
    assert torch.equal(ref, got)
    assert torch.isfinite(got.float()).all()


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("plane", DW_PLANES)
def test_dwconv_bwd_data_mul_identity_and_in_place_prior(plane, dt):
    """k = 7 with the identity term, and prior == dx (the in-place accumulate it replaces)."""
    kk = K()
    B, (H, W), C = 2, plane, 24
    P = B * H * W
    dy, mul, prior = (rnd(P, C, dt=dt, seed=s) for s in (1, 2, 3))
    w = rnd(C, 1, 7, 7, seed=4) / 7
    dg = prior.clone()
    kk.dwconv_bwd_data(dy, (B, H, W), w, 7, add_identity=True, dx=dg, accumulate=True)
    ref = kk.scale_mul(dg, mul=mul)
    dx = prior.clone()
    kk.dwconv_bwd_data_mul(dy, (B, H, W), w, 7, mul, prior=dx, add_identity=True, dx=dx)
    assert torch.equal(ref, dx)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("k", [3, 7])
def test_dwconv_bwd_data_without_the_fold_is_unchanged(k, dt):
    """dfm_dwconv_bwd_data (prior and mul absent in the kernel) against float64 at the existing bound, and
    bit-equal to the folded entry point with a multiplier of ones (round(round(v) * 1) = round(v))."""
    kk = K()
    B, H, W, C = 2, 11, 13, 24
    dy = rnd(B * H * W, C, dt=dt, seed=1)
    w = rnd(C, 1, k, k, seed=2) / k
    dx = kk.dwconv_bwd_data(dy, (B, H, W), w, k)
    x4 = dy.double().view(B, H, W, C).permute(0, 3, 1, 2)
    ref = F.conv2d(x4, w.double().flip(2, 3), padding=k // 2, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    assert rel(dx, ref) < TOL[dt]
    ones = torch.ones_like(dy)
    assert torch.equal(dx, kk.dwconv_bwd_data_mul(dy, (B, H, W), w, k, ones))


# ------------------------------------------------------------------------------- D: layernorm_bwd_pool
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [8, 48, 128, 256])  # 8: off the vector LayerNorm path (the pair is issued)
@pytest.mark.parametrize("plane", [(3, 5), (7, 7), (11, 13), (30, 40)])
@pytest.mark.parametrize("dres", [False, True])
def test_layernorm_bwd_pool_bit_equal_to_pair(plane, C, dres, dt):
    k = K()
    B, (H, W) = 2, plane
    P = B * H * W
    x, dy = rnd(P, C, dt=dt, seed=1), rnd(P, C, dt=dt, seed=2)
    res = rnd(P, C, dt=dt, seed=3) if dres else None
    pooled = rnd(B * 49, 3 * C, dt=dt, seed=4)[:, 2 * C:]  # a column block, as dpooled[:, C:] is
    gam = torch.rand(C, device=DEV) + 0.5
    _, mu, rstd = k.layernorm(x, gam, torch.zeros(C, device=DEV))
    summed = dy.clone()
    k.pool7_bwd(pooled, (B, H, W), dx=summed, accumulate=True)
    ref = k.layernorm_bwd(x, summed, gam, mu, rstd, dres=res)
    got = k.layernorm_bwd_pool(x, dy.clone(), gam, mu, rstd, pooled, (B, H, W), dres=res)
    torch.cuda.synchronize()
    for name, a, b in zip(("dx", "dgamma", "dbeta"), ref, got):
        assert torch.equal(a, b), name
        assert torch.isfinite(b.float()).all(), name


def test_layernorm_bwd_pool_one_launch_on_the_vector_path():
    """On the vector path the fold is one first-stage launch (no pool kernel) and dy is left as it was."""
    k = K()
    B, H, W, C = 2, 11, 13, 48
    x, dy = rnd(B * H * W, C, dt=torch.bfloat16, seed=1), rnd(B * H * W, C, dt=torch.bfloat16, seed=2)
    pooled = rnd(B * 49, C, dt=torch.bfloat16, seed=3)
    gam = torch.rand(C, device=DEV) + 0.5
    _, mu, rstd = k.layernorm(x, gam, torch.zeros(C, device=DEV))
    keep = dy.clone()
    from kernel_variants import Trace
    with Trace() as t:
        k.layernorm_bwd_pool(x, dy, gam, mu, rstd, pooled, (B, H, W))
    assert t.launched == ["ln_bwd_vec_kernel<unsigned short, 8, 1>", "partial_sum_kernel<1>"], t.launched
    assert torch.equal(dy, keep)


# ------------------------------------------------------------------------------- E: pool7_pair
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C1,C2", [(16, 8), (256, 128)])
@pytest.mark.parametrize("plane", [(3, 5), (11, 13)])
def test_pool7_pair_bit_equal_to_two_calls(plane, C1, C2, dt):
    k = K()
    B, (H, W) = 2, plane
    x1, x2 = rnd(B * H * W, C1, dt=dt, seed=1), rnd(B * H * W, C2, dt=dt, seed=2)
    ref = torch.zeros(B * 49, C1 + C2, device=DEV, dtype=dt)
    got = torch.zeros_like(ref)
    k.pool7(x1, (B, H, W), out=ref[:, :C1])
    k.pool7(x2, (B, H, W), out=ref[:, C1:])
    k.pool7_pair(x1, x2, (B, H, W), got[:, :C1], got[:, C1:])
    torch.cuda.synchronize()
    assert torch.equal(ref, got)
    assert rel(got[:, :C1], F.adaptive_avg_pool2d(x1.double().view(B, H, W, C1).permute(0, 3, 1, 2), 7)
               .permute(0, 2, 3, 1).reshape(-1, C1)) < TOL[dt]


# ------------------------------------------------------------------------------- the Block
B_, H_, W_, C_ = 2, 11, 13, 32
BLOCK_CASES = {"window7": dict(window=7, drop_depth=False), "window0": dict(window=0, drop_depth=False),
               "window7_drop_depth": dict(window=7, drop_depth=True)}
MASKS = ([1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 1.0])  # per-sample DropPath keep masks, a zero in each call


def make_block(case, droppath):
    from dformer_amd.encoder import Block
    blk = Block(index=0, dim=C_, num_head=1, mlp_ratio=4, block_index=1, window=BLOCK_CASES[case]["window"],
                dropout_layer=dict(type="DropPath", drop_prob=0.25 if droppath else 0.0),
                drop_depth=BLOCK_CASES[case]["drop_depth"])
    sd = blk.state_dict()
    vals = gen.state_dict_values([(n, v.shape) for n, v in sd.items()])
    blk.load_state_dict({n: torch.from_numpy(np.asarray(v)).float() for n, v in vals.items()})
    return blk


def run_python(case, droppath, dt, fold, monkeypatch):
    """The autograd Block (AttentionFn and both ConvFFNFn) forward + backward; every output and gradient."""
    from dformer_amd import functional as Fn
    monkeypatch.setattr(Fn, "FOLD_BWD_PASSES", fold)
    blk = make_block(case, droppath).to(DEV)
    Fn.invalidate_weights()
    blk.train()
    if droppath:
        blk.drop_path_masks = [torch.tensor(m) for m in MASKS]
    tag = "bwd_passes_" + case
    x = torch.from_numpy(gen.normal(tag + "/x", (B_, H_, W_, C_))).to(DEV, dt).requires_grad_()
    xe = torch.from_numpy(gen.normal(tag + "/xe", (B_, H_, W_, C_ // 2))).to(DEV, dt).requires_grad_()
    y, ye = blk(x, xe)
    gy = torch.from_numpy(gen.normal(tag + "/gy", y.shape)).to(DEV, dt)
    gye = torch.from_numpy(gen.normal(tag + "/gye", ye.shape)).to(DEV, dt)
    torch.autograd.backward([y, ye], [gy, gye])
    torch.cuda.synchronize()
    out = {"y": y.detach(), "ye": ye.detach(), "dx": x.grad, "dxe": xe.grad}
    out.update({n: p.grad for n, p in blk.named_parameters() if p.grad is not None})
    return out


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("droppath", [False, True], ids=["keep", "droppath"])
@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_fold_bit_equal(case, droppath, dt, monkeypatch):
    """Every output and every gradient of the Block, FOLD_BWD_PASSES True against False."""
    ref = run_python(case, droppath, dt, False, monkeypatch)
    got = run_python(case, droppath, dt, True, monkeypatch)
    assert ref.keys() == got.keys() and len(ref) > 20
    differ = [n for n in ref if not torch.equal(ref[n], got[n])]
    assert not differ, differ
    assert all(torch.isfinite(t.float()).all() for t in got.values())


def test_block_fold_calls_the_folded_kernels(monkeypatch):
    """With the switch on the step calls the four folded entry points (and not the passes they replace)."""
    from dformer_amd import kernels as Kk
    calls = []
    for fn in ("residual_bwd2", "dwconv_bwd_data_mul", "layernorm_bwd_pool", "pool7_pair", "pool7", "scale_mul"):
        orig = getattr(Kk, fn)

        def counted(*a, _o=orig, _n=fn, **kw):
            calls.append(_n)
            return _o(*a, **kw)
        monkeypatch.setattr(Kk, fn, counted)
    run_python("window7", False, torch.bfloat16, True, monkeypatch)
    assert [calls.count(n) for n in ("residual_bwd2", "dwconv_bwd_data_mul", "layernorm_bwd_pool", "pool7_pair")] == \
        [1, 1, 1, 1], calls
    assert "pool7" not in calls and "scale_mul" not in calls, calls


@pytest.mark.parametrize("dt,tol", [(torch.float32, 1e-3), (torch.bfloat16, 2e-2)], ids=["fp32", "bf16"])
@pytest.mark.parametrize("droppath", [False, True], ids=["keep", "droppath"])
@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_capi_matches_unfolded_python_route(case, droppath, dt, tol, monkeypatch):
    """dfm_block_fwd / dfm_block_bwd (block.cpp makes the same four substitutions) against the Python route
    with FOLD_BWD_PASSES False, at test_block_capi_gpu.py's tolerances (1e-3 in fp32, 2e-2 in bf16: the two
    routes group their GEMMs differently, so their split-K sums differ in order)."""
    import test_block_capi_gpu as capi
    from goldens import rel_err
    ref = run_python(case, droppath, dt, False, monkeypatch)
    blk = make_block(case, droppath)
    last = BLOCK_CASES[case]["drop_depth"]
    tag = "bwd_passes_" + case
    monkeypatch.setattr(capi, "_meta", lambda name: ({"y_e": True}, blk, (B_, H_, W_, C_, 1, last, 0.25)))
    keep = 0.75
    masks = [[m / keep for m in ms] for ms in MASKS] if droppath else None
    _, _, y, ye, dx, dxe, grads = capi.run_capi(tag, dt, stack_qcl=True, droppath=masks)
    pairs = [("y", y, ref["y"]), ("ye", ye, ref["ye"]), ("dx", dx, ref["dx"]), ("dxe", dxe, ref["dxe"])]
    pairs += [(n, grads[n], ref[n]) for n in grads]
    assert len(pairs) > 20
    bad = {}
    for n, a, b in pairs:
        a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
        e = rel_err(a, b) if float(b.abs().max()) > 0 else float(a.abs().max())
        if not math.isfinite(e) or e > tol:
            bad[n] = e
    assert not bad, bad
