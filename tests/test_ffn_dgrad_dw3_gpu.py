"""dfm_ffn_dgrad_dw3_bwd (the ConvFFN backward's fc2 input gradient times GELU' fused into the 3x3 backward)
against a float64 reference and against the pair of kernels it replaces (GPU)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.bfloat16: 2e-2, torch.float16: 3e-3}  # tests/test_kernels_gpu.py
ROUND = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}  # one output rounding, relative
# (B, H, W, C, hidden): a plane smaller than one strip and one chunk; an odd plane of two images; more units
# than one grid round; K = 128 with a ragged last strip and last chunk; four channel slices; one full stage-0
# depth plane of many chunks
SHAPES = [(1, 2, 3, 32, 128), (2, 5, 7, 64, 256), (3, 15, 20, 64, 128), (1, 33, 41, 128, 256), (1, 30, 40, 64, 512),
          (1, 120, 160, 32, 256)]
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from dformer_amd import kernels  # noqa: F401
    yield
    _CACHE.clear()  # the shared cases' tensors


def K():
    from dformer_amd import kernels
    return kernels


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def make_inputs(dt, B, H, W, C, R, zero_df=False):
    """Rounded operands as strided views (ld > width): df, W2, gp = GELU'(randn), h, wpos, and an output view."""
    g = torch.Generator(device=DEV).manual_seed(1000 * B + 100 * H + W + C + R)
    P = B * H * W

    def randn(*s):
        return torch.randn(*s, device=DEV, generator=g)
    df = randn(P, C + 8).to(dt)[:, :C]
    if zero_df:
        df.zero_()
    gp = gelu_grad(randn(P, R + 16)).to(dt)[:, 16:]
    h = randn(P, R + 8).to(dt)[:, 8:]
    w2 = (randn(C, R) / math.sqrt(C)).to(dt)
    wpos = randn(R, 1, 3, 3) / 3
    dh = torch.full((P, R + 24), 7.0, device=DEV, dtype=dt)[:, 8:8 + R]
    return df, w2, gp, h, wpos, dh


def reference64(dt, shape, df, w2, gp, h, wpos, identity=True):
    """dhpre in float64 from the rounded inputs, rounded to dt, then the transposed conv (+ identity) in float64."""
    B, H, W = shape
    R = w2.shape[1]
    dhpre = ((df.double() @ w2.double()) * gp.double()).to(dt).double()
    hr = h.double().reshape(B, H, W, R).permute(0, 3, 1, 2).contiguous().requires_grad_()
    wr = wpos.double().requires_grad_()
    br = torch.zeros(R, device=DEV, dtype=torch.float64, requires_grad=True)
    hpre = F.conv2d(hr, wr, br, padding=1, groups=R)
    if identity:
        hpre = hpre + hr
    hpre.backward(dhpre.reshape(B, H, W, R).permute(0, 3, 1, 2))
    return hr.grad.permute(0, 2, 3, 1).reshape(B * H * W, R), wr.grad, br.grad


_CACHE = {}


def case(dt, shp):
    """One fused call, the pair and the float64 reference per (dtype, shape), shared by the checks."""
    key = (dt, shp)
    if key not in _CACHE:
        k = K()
        B, H, W, C, R = shp
        df, w2, gp, h, wpos, dh = make_inputs(dt, *shp)
        assert k.ffn_dgrad_dw3_supported(dt, (B, H, W), C, R)
        _, dw, db = k.ffn_dgrad_dw3_bwd(df, w2, gp, h, (B, H, W), wpos, dh=dh)
        dhpre = k.linear_dgrad(df, w2, mul=gp)
        pair = k.dwconv_bwd(h, dhpre, (B, H, W), wpos, 3, add_identity=True)
        ref = reference64(dt, (B, H, W), df, w2, gp, h, wpos)
        torch.cuda.synchronize()
        _CACHE[key] = ((df, w2, gp, h, wpos), (dh, dw, db), pair, ref)
    return _CACHE[key]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shp", SHAPES)
def test_vs_float64(dt, shp):
    _, (dh, dw, db), _, (rdh, rdw, rdb) = case(dt, shp)
    errs = rel(dh, rdh), rel(dw, rdw), rel(db, rdb)
    print(f"{shp} {dt}: dh {errs[0]:.3e} dw {errs[1]:.3e} db {errs[2]:.3e}")
    assert errs[0] < TOL[dt] and errs[2] < TOL[dt] and errs[1] < 2 * TOL[dt], errs


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shp", SHAPES)
def test_vs_pair(dt, shp):
    """The only legitimate difference is fp32 accumulation order before the same rounding: the fused dh error
    against float64 exceeds the pair's by at most one output rounding; dw / db to fp32 summation order."""
    _, (dh, dw, db), (pdh, pdw, pdb), (rdh, _, _) = case(dt, shp)
    ef, ep = rel(dh, rdh), rel(pdh, rdh)
    print(f"{shp} {dt}: dh error fused {ef:.3e} pair {ep:.3e}; dw vs pair {rel(dw, pdw):.3e} db {rel(db, pdb):.3e}")
    assert ef <= ep + ROUND[dt], (ef, ep)
    assert rel(dw, pdw) < 1e-5 and rel(db, pdb) < 1e-5


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shp", SHAPES)
def test_reproducible(dt, shp):
    (df, w2, gp, h, wpos), (dh, dw, db), _, _ = case(dt, shp)
    B, H, W, C, R = shp
    dh2, dw2, db2 = K().ffn_dgrad_dw3_bwd(df, w2, gp, h, (B, H, W), wpos)
    assert torch.equal(dh, dh2) and torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shp", SHAPES)
def test_zero_gradient(dt, shp):
    """df = 0 gives exactly zero dh, dw, db (uninitialised ring rows or halo would not)."""
    B, H, W, C, R = shp
    df, w2, gp, h, wpos, dh = make_inputs(dt, *shp, zero_df=True)
    _, dw, db = K().ffn_dgrad_dw3_bwd(df, w2, gp, h, (B, H, W), wpos, dh=dh)
    assert not dh.any() and not dw.any() and not db.any()


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_without_identity(dt):
    """add_identity = 0 (a plain 3x3 depthwise conv behind the GEMM): the same gates as with the identity."""
    k = K()
    shp = (2, 5, 7, 64, 256)
    B, H, W, C, R = shp
    df, w2, gp, h, wpos, dh = make_inputs(dt, *shp)
    _, dw, db = k.ffn_dgrad_dw3_bwd(df, w2, gp, h, (B, H, W), wpos, add_identity=False, dh=dh)
    pdh, pdw, pdb = k.dwconv_bwd(h, k.linear_dgrad(df, w2, mul=gp), (B, H, W), wpos, 3, add_identity=False)
    rdh, rdw, rdb = reference64(dt, (B, H, W), df, w2, gp, h, wpos, identity=False)
    ef, ep = rel(dh, rdh), rel(pdh, rdh)
    assert ef < TOL[dt] and rel(db, rdb) < TOL[dt] and rel(dw, rdw) < 2 * TOL[dt]
    assert ef <= ep + ROUND[dt], (ef, ep)
    assert rel(dw, pdw) < 1e-5 and rel(db, pdb) < 1e-5


def test_supported_looks_at_the_operands():
    """Rows that are not 16-byte vectors (odd row stride, misaligned pointer, strided inner dimension) are not
    supported, so a caller takes the pair instead of meeting DFM_ERR_ARG."""
    k = K()
    dt, shp = torch.bfloat16, (1, 6, 9, 32, 128)
    B, H, W, C, R = shp
    df, w2, gp, h, wpos, dh = make_inputs(dt, *shp)
    assert k.ffn_dgrad_dw3_supported(dt, (B, H, W), C, R, operands=(df, w2, gp, h, dh))
    odd_ld = torch.zeros(B * H * W, R + 4, device=DEV, dtype=dt)[:, :R]
    misaligned = torch.zeros(B * H * W, R + 8, device=DEV, dtype=dt)[:, 4:4 + R]
    strided = torch.zeros(B * H * W, 2 * R, device=DEV, dtype=dt)[:, ::2]
    for bad in (odd_ld, misaligned, strided):
        assert not k.ffn_dgrad_dw3_supported(dt, (B, H, W), C, R, operands=(df, w2, bad, h))
        assert not k.ffn_dgrad_dw3_supported(dt, (B, H, W), C, R, operands=(df, w2, gp, bad))
    with pytest.raises(RuntimeError, match="16-byte"):
        k.ffn_dgrad_dw3_bwd(df, w2, odd_ld, h, (B, H, W), wpos, dh=dh)
    torch.cuda.synchronize()
    assert torch.all(dh == 7.0)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_unsupported_shape_is_an_error_before_any_launch(dt):
    k = K()
    B, H, W, C, R = 1, 6, 9, 32, 136
    assert not k.ffn_dgrad_dw3_supported(dt, (B, H, W), C, R)
    assert not k.ffn_dgrad_dw3_supported(torch.float32, (B, H, W), 32, 128)
    df, w2, gp, h, wpos, dh = make_inputs(dt, B, H, W, C, R)
    k.ACCOUNT = []
    k.trace(1)
    try:
        with pytest.raises(RuntimeError, match="unsupported"):
            k.ffn_dgrad_dw3_bwd(df, w2, gp, h, (B, H, W), wpos, dh=dh)
        launched = k.lib.dfm_trace_take(k._FUNCS, 64)
    finally:
        k.trace(0)
        k.ACCOUNT = None
    torch.cuda.synchronize()
    assert launched == 0
    assert torch.all(dh == 7.0)
