"""Every kernel instantiation of the hot-path families, pinned: one table of cases, each of which
names the exact set of kernels its call must launch (checked with the library's launch tracer) and
checks every output against an fp64 reference of the same operation on the same rounded operands.

The declared names are the ledger's "pinned" side (tests/test_kernel_variants_cpu.py); they are
computed here from a Python transcription of the dispatch rules, so a routing threshold that moves
makes the case that loses its kernel fail with the name it got instead.

Gates. Linear operations (GEMM, depthwise convolution, pooling, bilinear resize) are checked element
by element against the fp64 reference r:  |y - r| <= u_out |r| + 2 n 2^-24 S,  with S the same operation
on the absolute values, n the number of accumulated terms per output and u_out the unit roundoff of
the output type: the worst-case fp32 accumulation bound, doubled for the MFMA's internal rounding
and the epilogue. Two further terms are derived and named where they are added: the part of the
output's half ulp that u_out |r| leaves out (bf16 only: 2^-9 is the half ulp at the top of a binade,
a correctly rounded bf16 result errs by up to 2^-8 |r| at the bottom; see _check), and for bilinear
resize the rounding of its fp32 source coordinate (see bilinear_case).
LayerNorm and attention keep their family's gates of test_kernels_gpu.py (error relative to the
largest reference element), now against fp64.
"""
import math
import zlib
from typing import Callable, NamedTuple

import pytest
import torch
import torch.nn.functional as F

import kernel_variants as kv

DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
TN = {F32: "float", BF16: "unsigned short", F16: "f16_t"}  # as a demangled name spells them (bf16_t is an alias)
SHORT = {F32: "f32", BF16: "bf16", F16: "f16"}
U_OUT = {F32: 2.0 ** -24, BF16: 2.0 ** -9, F16: 2.0 ** -11}
# u_out -> (significand bits, smallest normal exponent) of that output type (see _check)
ROUNDING = {2.0 ** -24: (24, -126), 2.0 ** -9: (8, -126), 2.0 ** -11: (11, -14)}
# the families' gates of test_kernels_gpu.py (relative to the largest reference element)
TOL = {F32: 2e-5, BF16: 2e-2, F16: 3e-3}
ATTN_TOL = {F32: 2e-5, BF16: 6e-3, F16: 1.5e-3}
PSUM = {0: "partial_sum_kernel<0>", 1: "partial_sum_kernel<1>", 2: "partial_sum_kernel<2>"}
BIG = 1 << 22  # reference tensors above this many elements are computed with torch fp64 on the GPU


class Case(NamedTuple):
    id: str
    family: str                  # source file of the kernels it pins
    names: frozenset             # the kernels the call must launch, all of them
    run: Callable                # () -> (launched names, [check])


class Lin(NamedTuple):           # elementwise bound of a linear operation
    what: str
    got: torch.Tensor
    ref: torch.Tensor
    S: torch.Tensor
    n: int
    u: float
    extra: object = None         # a further derived term of the bound (tensor), named where it is built


class Rel(NamedTuple):           # error relative to the largest reference element
    what: str
    got: torch.Tensor
    ref: torch.Tensor
    tol: float


class Same(NamedTuple):          # bytes the call must not have touched
    what: str
    got: torch.Tensor
    ref: torch.Tensor


SPLIT = {}  # case id -> (forward names, backward names) of a case that makes a forward and a backward call


def K():
    from dformer_amd import kernels
    return kernels


def gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def rnd(g, shape, dt, scale=1.0, shift=0.0):
    """Fixed-seed CPU normal data, rounded to the storage type (the operands are exact in it)."""
    return (torch.randn(shape, generator=g) * scale + shift).to(dt)


SENT = 7.0


def strided(t, ld):
    """t [rows, cols] on the GPU as a view of row stride ld (the pad columns hold a sentinel)."""
    rows, cols = t.shape
    buf = torch.full((rows, ld), SENT, dtype=t.dtype, device=DEV)
    buf[:, :cols] = t.to(DEV)
    return buf[:, :cols], buf


def pad_ok(what, buf, cols):
    return Same(what + " pad columns", buf[:, cols:], torch.full_like(buf[:, cols:], SENT))


def up8(n):
    return (n + 7) // 8 * 8


def d64(t, dev="cpu"):
    return t.to(dev).double()


# ================================================================================ single GEMM
def gemm_tile(Nw):
    """pick_tile + the tile's wave layout: (BN, NW, WAVES_M)."""
    return (32, 4, 4) if Nw <= 32 else ((64, 4, 2) if Nw <= 64 else (128, 8, 2))


def gemm_route(dt, M, N, K, ak, bk, aligned, split_k=0):
    """The kernels dfm_gemm launches (gemm_typed's rules: pick_tile, choose_splits, small_k, wide_eligible,
    route, launch_depth) for a plain descriptor: a single matrix, no colsum, alpha 1, output in the operand
    type, at most one epilogue tile."""
    t, es = TN[dt], (4 if dt == F32 else 2)
    BN, NW, WM = gemm_tile(N)
    tiles = -(-M // 128) * -(-N // BN)
    if split_k >= 1:
        splits = split_k
    elif K < 1024 or tiles >= 256:
        splits = 1
    else:
        s, splits = min(-(-256 // tiles), K // 512), 1
        while 2 * splits <= s and splits < 1024:
            splits *= 2
    small_k = K <= (128 if es == 2 else 64)
    glds_ok = es == 2 and ak and aligned
    if glds_ok and split_k < 1:
        splits = 1
    glds_ok = glds_ok and -(-K // splits) >= 128
    reduce = []
    if splits > 1:
        reduce = [f"splitk_reduce_kernel<{t}, {4 if splits >= 8 else 1}>"]
    tf = {True: "true", False: "false"}
    if es == 2:
        if (ak and splits == 1 and aligned and K % 16 == 0 and 32 <= K <= 128 and N % 8 == 0 and M >= 65536 and
                N >= 144):
            return [f"gemm_wide_kernel<{t}, {-(-K // 32) * 32}, {tf[bk]}>"]
        route = ak and ((not (N > 512 and K <= 128)) if bk else K >= 128)
        if glds_ok and route:
            if BN == 32:
                cfg = "128, 32, 4, 4, true, {}, 2, 3"
            elif splits == 1 and M >= 65536 and N >= 512 and K >= 512:
                cfg = "128, 128, 8, 2, true, {}, 2, 2"
            else:
                cfg = "64, 64, 4, 2, true, {}, 2, 4"
            return [f"gemm_glds_kernel<{t}, {cfg.format(tf[bk])}>"] + reduce
    if small_k:
        BK, depth = (32 if es == 2 else 16), 1
    else:
        BK = 64 if es == 2 else 32
        kper = -(-K // splits)
        blocks = tiles * splits
        depth = 2 if (kper >= 8 * BK and blocks <= 512) else 1
    return [f"gemm_kernel<{t}, 128, {BN}, {NW}, {WM}, {BK}, {tf[ak]}, {tf[bk]}, {depth}>"] + reduce


def gemm_case(cid, dt, M, N, Kd, ak, bk, aligned, split_k=0, epi=None):
    """y = epi(A @ B + bias). A(m,k) is stored [M,K] (ak) or [K,M]; B(k,n) is stored [N,K] (bk) or [K,N].
    aligned: leading dimensions are multiples of 8 elements (with pad columns), else odd. epi: None,
    "mul" (times a tile), "res" (res + colscale * rowscale * (.)), "beta" (plus the old output)."""
    names = frozenset(gemm_route(dt, M, N, Kd, ak, bk, aligned, split_k))

    def run():
        g = gen(cid)
        big = M * N * Kd > 2e8
        rdev = DEV if big else "cpu"
        pad = (lambda c: up8(c) + 8) if aligned else (lambda c: up8(c) + 1)
        a0 = rnd(g, (M, Kd) if ak else (Kd, M), dt)
        b0 = rnd(g, (N, Kd) if bk else (Kd, N), dt)
        bias = torch.randn(N, generator=g)
        a, _ = strided(a0, pad(a0.shape[1]))
        b, _ = strided(b0, pad(b0.shape[1]))
        c0 = rnd(g, (M, N), dt)
        out, obuf = strided(c0, pad(N))
        A = d64(a0, rdev) if ak else d64(a0, rdev).t()
        Bm = d64(b0, rdev).t() if bk else d64(b0, rdev)
        ref = A @ Bm + d64(bias, rdev)
        S = A.abs() @ Bm.abs() + d64(bias, rdev).abs()
        n = Kd + 1
        kw = {}
        if epi == "mul":
            m0 = rnd(g, (M, N), dt)
            kw["mul"], _ = strided(m0, pad(N))
            kw["ldmul"] = kw["mul"].stride(0)
            ref, S, n = ref * d64(m0, rdev), S * d64(m0, rdev).abs(), n + 1
        elif epi == "res":
            r0 = rnd(g, (M, N), dt)
            kw["res"], _ = strided(r0, pad(N))
            kw["ldres"] = kw["res"].stride(0)
            cs, rs = torch.randn(N, generator=g), torch.randn(-(-M // 7), generator=g)
            kw.update(colscale=cs.to(DEV), rowscale=rs.to(DEV), rows_per_scale=7)
            f = d64(cs, rdev)[None, :] * d64(rs, rdev).repeat_interleave(7)[:M, None]
            ref, S, n = d64(r0, rdev) + f * ref, d64(r0, rdev).abs() + f.abs() * S, n + 3
        elif epi == "beta":
            kw["beta"] = 1.0
            ref, S, n = ref + d64(c0, rdev), S + d64(c0, rdev).abs(), n + 1
        with kv.Trace() as tr:
            K().gemm(a, b, M=M, N=N, K=Kd, a_kcontig=ak, b_kcontig=bk, lda=a.stride(0), ldb=b.stride(0), out=out,
                     ldc=out.stride(0), bias=bias.to(DEV), split_k=split_k, **kw)
        return tr.names, [Lin("y", out, ref, S, n, U_OUT[dt]), pad_ok("y", obuf, N)]

    return Case(cid, "gemm", names, run)


def gemm_cases():
    out = []
    for dt in DTYPES:
        s = SHORT[dt]
        two = dt != F32
        # K per k-loop kind: short (one BK-short chunk loop with a ragged tail), long at pipeline depth 1,
        # long at depth 2 (>= 8 chunks per block); M = 150 is two row tiles with a ragged tail
        kinds = {"short": 72 if two else 40, "long1": 200 if two else 100, "long2": 520 if two else 264}
        for N in (24, 56, 136):                       # one 32-column tile, one 64-column tile, two 128-column tiles
            for kind, Kd in kinds.items():
                for ak in (True, False):
                    for bk in (True, False):
                        for aligned in (True, False):
                            want_k = f"gemm_kernel<{TN[dt]}"
                            names = gemm_route(dt, 150, N, Kd, ak, bk, aligned)
                            if not names[0].startswith(want_k):
                                continue  # 16-bit aligned k-contiguous A, long K: the ring kernel (below)
                            cid = f"gemm-{s}-n{N}-{kind}-a{int(ak)}b{int(bk)}-{'al' if aligned else 'mis'}"
                            out.append(gemm_case(cid, dt, 150, N, Kd, ak, bk, aligned,
                                                 epi=None if aligned else "res"))
        # split-K combines (2 splits: one lane per output; 8 splits: four), weight-gradient layout
        for sk in (2, 8):
            for N in (24, 136):
                out.append(gemm_case(f"gemm-{s}-n{N}-split{sk}", dt, 150, N, 1100, False, False, True, split_k=sk))
        out.append(gemm_case(f"gemm-{s}-n136-split8-mis", dt, 150, 136, 1100, False, False, False, split_k=8))
        if not two:
            continue
        # the LDS-DMA ring kernel: 128x32 and 64x64 tiles, and 128x128 from 65,536 rows x 512 x 512
        for bk in (True, False):
            b_ = int(bk)
            out.append(gemm_case(f"gemm-{s}-ring32-b{b_}", dt, 150, 24, 200, True, bk, True, epi="mul"))
            out.append(gemm_case(f"gemm-{s}-ring64-b{b_}", dt, 150, 136, 200, True, bk, True, epi="res"))
            out.append(gemm_case(f"gemm-{s}-ring64-b{b_}-split2", dt, 150, 136, 1100, True, bk, True, split_k=2))
            out.append(gemm_case(f"gemm-{s}-ring128-b{b_}", dt, 65536 + 77, 520, 520, True, bk, True, epi="beta"))
            # the tall short-K kernel: K padded to 64 / 128 and exact at 32 / 96; two column slices, ragged
            for Kd, epi in ((32, None), (48, "mul"), (96, "res"), (112, "beta")):
                out.append(gemm_case(f"gemm-{s}-wide-k{Kd}-b{b_}", dt, 65536 + 77, 152, Kd, True, bk, True, epi=epi))
    return out


# ================================================================================ LayerNorm
def ln_geom(dt, C):
    """ln_vec_geom / pick_g: ("vec", G, NV) or ("scalar", G)."""
    V = 4 if dt == F32 else 8
    if C % V == 0 and C // V >= 4:
        nvec, G = C // V, 4
        while G < 64 and G < nvec:
            G *= 2
        NV = -(-nvec // G)
        if NV in (1, 2, 4):
            return ("vec", G, NV)
    G = 8
    while G < 64 and G * 8 < C:
        G *= 2
    return ("scalar", G)


def ln_case(dt, C, rows=301):
    geom = ln_geom(dt, C)
    t = TN[dt]
    if geom[0] == "vec":
        fwd, bwd = f"ln_fwd_vec_kernel<{t}, {geom[1]}, {geom[2]}>", f"ln_bwd_vec_kernel<{t}, {geom[1]}, {geom[2]}>"
    else:
        fwd, bwd = f"ln_fwd_kernel<{t}, {geom[1]}>", f"ln_bwd_kernel<{t}, {geom[1]}>"
    cid = f"ln-{SHORT[dt]}-c{C}"

    def run():
        g = gen(cid)
        k = K()
        ldp = up8(C) + 8  # row strides keep the vector alignment; C itself decides the path
        x0, dy0, dres0, base0 = rnd(g, (rows, C), dt, 2.0, 0.5), rnd(g, (rows, C), dt), rnd(g, (rows, C), dt), \
            rnd(g, (rows, C), dt)
        gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        x, _ = strided(x0, ldp)
        y, ybuf = strided(torch.zeros(rows, C, dtype=dt), ldp)
        dy, _ = strided(dy0, ldp)
        dres, _ = strided(dres0, ldp)
        dx, dxbuf = strided(base0, ldp)
        gd, bd = gam.to(DEV), bet.to(DEV)
        with kv.Trace() as t1:
            _, mean, rstd = k.layernorm(x, gd, bd, 1e-6, out=y)
        with kv.Trace() as t2:
            _, dg, db = k.layernorm_bwd(x, dy, gd, mean, rstd, dx=dx, accumulate=True, dres=dres)
        xr = d64(x0).requires_grad_()
        gr, br = d64(gam).requires_grad_(), d64(bet).requires_grad_()
        ref = F.layer_norm(xr, (C,), gr, br, 1e-6)
        ref.backward(d64(dy0))
        mu = d64(x0).mean(1)
        rs = 1.0 / (d64(x0).var(1, unbiased=False) + 1e-6).sqrt()
        tol = TOL[dt]
        checks = [Rel("y", y, ref.detach(), tol), pad_ok("y", ybuf, C),
                  # the statistics are fp32 sums over exact inputs whatever the storage type
                  Rel("mean", mean, mu, TOL[F32]), Rel("rstd", rstd, rs, TOL[F32]),
                  Rel("dx", dx, xr.grad + d64(dres0) + d64(base0), 2 * tol), pad_ok("dx", dxbuf, C),
                  Rel("dgamma", dg, gr.grad, 2 * tol), Rel("dbeta", db, br.grad, tol)]
        return (t1.names, t2.names), checks

    SPLIT[cid] = (frozenset([fwd]), frozenset([bwd, PSUM[1]]))
    return Case(cid, "layernorm", frozenset([fwd, bwd, PSUM[1]]), run)


def ln_cases():
    out = []
    # every vector geometry (G lanes per row, NV vectors per lane) and every scalar G; the scalar C are
    # no multiple of the vector width (4 elements for fp32, 8 for the 16-bit types)
    vec16 = [32, 56, 104, 200, 392, 776]          # (4,1) (8,1) (16,1) (32,1) (64,1) (64,2)
    vec32 = [16, 28, 52, 100, 196, 388, 780]      # the same and (64,4)
    scalar = [50, 101, 203, 515]                  # G = 8, 16, 32, 64
    for dt in DTYPES:
        for C in (vec32 if dt == F32 else vec16) + scalar:
            out.append(ln_case(dt, C))
    return out


# ================================================================================ pool7 / bilinear
def _pool_mat(n):
    """[7, n] adaptive average pooling matrix (bins floor(i n / 7) .. ceil((i+1) n / 7))."""
    m = torch.zeros(7, n, dtype=torch.float64)
    for i in range(7):
        lo, hi = (i * n) // 7, -(-((i + 1) * n) // 7)
        m[i, lo:hi] = 1.0 / (hi - lo)
    return m


def _bilinear_mats(n_in, n_out):
    """([n_out, n_in] interpolation matrix of align_corners=False, [n_out, n_in] 0/1 matrix of the taps that
    a source coordinate off by a rounding error could read)."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    near = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        src = max((o + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = src - i0
        m[o, i0] += 1.0 - l1
        m[o, i1] += l1
        for i in range(n_in):
            if abs(i - src) < 1.001:
                near[o, i] = 1.0
    return m, near


def _sep(mh, mw, x4):
    """y[b,o,p,c] = sum mh[o,h] mw[p,w] x[b,h,w,c]."""
    return torch.einsum("oh,pw,bhwc->bopc", mh, mw, x4)


def _nnz(m, dim):
    return int((m != 0).sum(dim).max().item())


def pool_case(dt, C, B=2, H=17, W=23):
    t = TN[dt]
    vec = C % 8 == 0
    fwd = f"pool7_fwd_vec_kernel<{t}>" if vec and C <= 2048 else f"pool7_fwd_kernel<{t}>"
    bwd = f"pool7_bwd_vec_kernel<{t}>" if vec else f"pool7_bwd_kernel<{t}>"
    cid = f"pool7-{SHORT[dt]}-c{C}"

    def run():
        g, k = gen(cid), K()
        ldp = up8(C) + 8
        x0, dy0, base0 = rnd(g, (B * H * W, C), dt), rnd(g, (B * 49, C), dt), rnd(g, (B * H * W, C), dt)
        x, _ = strided(x0, ldp)
        dy, _ = strided(dy0, ldp)
        y, ybuf = strided(torch.zeros(B * 49, C, dtype=dt), ldp)
        dx, dxbuf = strided(base0, ldp)
        with kv.Trace() as t1:
            k.pool7(x, (B, H, W), out=y)
        with kv.Trace() as t2:
            k.pool7_bwd(dy, (B, H, W), dx=dx, accumulate=True)
        mh, mw = _pool_mat(H), _pool_mat(W)
        x4, dy4 = d64(x0).view(B, H, W, C), d64(dy0).view(B, 7, 7, C)
        ref, S = _sep(mh, mw, x4), _sep(mh, mw, x4.abs())
        # the project's definition of the operation, once: the matrices are torch's adaptive pooling
        tref = F.adaptive_avg_pool2d(x4.permute(0, 3, 1, 2), 7).permute(0, 2, 3, 1)
        assert (ref - tref).abs().max().item() < 1e-12
        rb = _sep(mh.t(), mw.t(), dy4) + d64(base0).view(B, H, W, C)
        Sb = _sep(mh.t(), mw.t(), dy4.abs()) + d64(base0).view(B, H, W, C).abs()
        nf = _nnz(mh, 1) * _nnz(mw, 1) + 1          # window sum, then the division
        nb = _nnz(mh, 0) * _nnz(mw, 0) * 2 + 1      # a division and an add per window, the accumulate
        return (t1.names, t2.names), [
            Lin("y", y, ref.reshape(-1, C), S.reshape(-1, C), nf, U_OUT[dt]), pad_ok("y", ybuf, C),
            Lin("dx", dx, rb.reshape(-1, C), Sb.reshape(-1, C), nb, U_OUT[dt]), pad_ok("dx", dxbuf, C)]

    SPLIT[cid] = (frozenset([fwd]), frozenset([bwd]))
    return Case(cid, "attention", frozenset([fwd, bwd]), run)


def bilinear_case(dt, C, hi, ho, B=2):
    t = TN[dt]
    vec = C % 8 == 0
    taps_fit = 2 * (ho[0] // hi[0]) + 6 <= 64 and 2 * (ho[1] // hi[1]) + 6 <= 64 and ho[0] >= hi[0] and ho[1] >= hi[1]
    fwd = f"bilinear_fwd_vec_kernel<{t}>" if vec else f"bilinear_fwd_kernel<{t}>"
    bwd = f"bilinear_bwd_vec_kernel<{t}>" if vec and C <= 2048 and taps_fit else f"bilinear_bwd_kernel<{t}>"
    cid = f"bilinear-{SHORT[dt]}-c{C}-{hi[0]}x{hi[1]}-{ho[0]}x{ho[1]}"

    def run():
        g, k = gen(cid), K()
        ldp = up8(C) + 8
        ni, no = B * hi[0] * hi[1], B * ho[0] * ho[1]
        x0, dy0, ybase0, dxbase0 = rnd(g, (ni, C), dt), rnd(g, (no, C), dt), rnd(g, (no, C), dt), rnd(g, (ni, C), dt)
        x, _ = strided(x0, ldp)
        dy, _ = strided(dy0, ldp)
        y, ybuf = strided(ybase0, ldp)
        dx, dxbuf = strided(dxbase0, ldp)
        with kv.Trace() as t1:
            k.bilinear(x, hi, ho, B, out=y, accumulate=True)
        with kv.Trace() as t2:
            k.bilinear_bwd(dy, hi, ho, B, dx=dx, accumulate=True)
        (mh, nh), (mw, nw) = _bilinear_mats(hi[0], ho[0]), _bilinear_mats(hi[1], ho[1])
        x4, dy4 = d64(x0).view(B, *hi, C), d64(dy0).view(B, *ho, C)
        yb, dxb = d64(ybase0).view(B, *ho, C), d64(dxbase0).view(B, *hi, C)
        tref = F.interpolate(x4.permute(0, 3, 1, 2), ho, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        assert (_sep(mh, mw, x4) - tref).abs().max().item() < 1e-12
        ref, S = _sep(mh, mw, x4) + yb, _sep(mh, mw, x4.abs()) + yb.abs()
        rb, Sb = _sep(mh.t(), mw.t(), dy4) + dxb, _sep(mh.t(), mw.t(), dy4.abs()) + dxb.abs()
        # The kernels compute the source coordinate scale * (o + 0.5) - 0.5 in fp32: the rounding of the
        # scale, of the product and of the difference move it by at most 3 * 2^-24 * (n_in + 1), and each
        # of the two taps' weights with it; a product of two weights moves by the sum over both axes. The
        # term multiplies the unweighted sum of |x| over the taps such a coordinate can read.
        eps = 4 * 2.0 ** -24 * ((hi[0] + 1) + (hi[1] + 1))
        Ef, Eb = eps * _sep(nh, nw, x4.abs()), eps * _sep(nh.t(), nw.t(), dy4.abs())
        nf = 4 * 2 + 1                                  # 4 taps, a weight product each, the accumulate
        nb = _nnz(nh, 0) * _nnz(nw, 0) * 2 + 1
        return (t1.names, t2.names), [
            Lin("y", y, ref.reshape(-1, C), S.reshape(-1, C), nf, U_OUT[dt], Ef.reshape(-1, C)), pad_ok("y", ybuf, C),
            Lin("dx", dx, rb.reshape(-1, C), Sb.reshape(-1, C), nb, U_OUT[dt], Eb.reshape(-1, C)),
            pad_ok("dx", dxbuf, C)]

    SPLIT[cid] = (frozenset([fwd]), frozenset([bwd]))
    return Case(cid, "attention", frozenset([fwd, bwd]), run)


def pool_bilinear_cases():
    out = []
    for dt in DTYPES:
        for C in (24, 20):  # 8-channel vectors / scalar (C no multiple of 8)
            out.append(pool_case(dt, C))
            out.append(bilinear_case(dt, C, (7, 9), (15, 20)))    # upscale (source coordinates hit integers)
            out.append(bilinear_case(dt, C, (15, 20), (7, 9)))    # downscale: the backward's scalar kernel
    return out


# ================================================================================ pooled attention
def attn_names(dt, dh, aligned=True):
    t = TN[dt]
    if dt != F32 and dh % 16 != 0 and dh <= 48:
        dp = -(-dh // 16) * 16
        rp = "head_repack4_kernel" if dh % 4 == 0 else "head_repack_kernel"
        return (frozenset([rp, f"attn_fwd_mfma_kernel<{t}, {dp}>", f"attn_fwd_combine_v4_kernel<{t}>"]),
                frozenset([rp, f"attn_bwd_mfma_kernel<{t}, {dp}>", f"attn_dq_reduce_v4_kernel<{t}>"]))
    if dt != F32 and dh in (16, 32, 48) and aligned:
        return (frozenset([f"attn_fwd_mfma_kernel<{t}, {dh}>", f"attn_fwd_combine_v4_kernel<{t}>"]),
                frozenset([f"attn_bwd_mfma_kernel<{t}, {dh}>", f"attn_dq_reduce_v4_kernel<{t}>"]))
    return (frozenset([f"attn_fwd_chunk_kernel<{t}>", f"attn_fwd_combine_kernel<{t}>"]),
            frozenset([f"attn_bwd_chunk_kernel<{t}>", f"attn_dq_reduce_kernel<{t}>"]))


def attn_case(dt, N, dh, B=2, heads=2, aligned=True):
    fwd, bwd = attn_names(dt, dh, aligned)
    cid = f"attn-{SHORT[dt]}-n{N}-dh{dh}" + ("" if aligned else "-mis")

    def run():
        g, k = gen(cid), K()
        C2 = heads * dh
        ldp = up8(C2) + 8 if aligned else up8(C2) + 4  # (+4: rows are not 16-byte aligned for 16-bit types)
        q0, k0, v0, do0 = rnd(g, (B * 49, C2), dt), rnd(g, (B * N, C2), dt), rnd(g, (B * N, C2), dt), \
            rnd(g, (B * 49, C2), dt)
        q, _ = strided(q0, ldp)
        kk, _ = strided(k0, ldp)
        v, _ = strided(v0, ldp)
        do, _ = strided(do0, ldp)
        z = torch.zeros
        o, obuf = strided(z(B * 49, C2, dtype=dt), ldp)
        dq, dqbuf = strided(z(B * 49, C2, dtype=dt), ldp)
        dk, dkbuf = strided(z(B * N, C2, dtype=dt), ldp)
        dv, dvbuf = strided(z(B * N, C2, dtype=dt), ldp)
        scale = dh ** -0.5
        with kv.Trace() as t1:
            _, lse = k.pooled_attn(q, kk, v, B, heads, N, dh, scale, out=o)
        with kv.Trace() as t2:
            k.pooled_attn_bwd(q, kk, v, o, do, lse, B, heads, N, dh, scale, dq, dk, dv)

        def heads_of(t, n):
            return d64(t).view(B, n, heads, dh).permute(0, 2, 1, 3)

        qr, kr, vr = (heads_of(q0, 49).requires_grad_(), heads_of(k0, N).requires_grad_(),
                      heads_of(v0, N).requires_grad_())
        ref = ((qr * scale) @ kr.transpose(-2, -1)).softmax(-1) @ vr
        ref.backward(heads_of(do0, 49))

        def rows_of(t, n):
            return t.permute(0, 2, 1, 3).reshape(B * n, C2)

        tol = ATTN_TOL[dt]
        return (t1.names, t2.names), [
            Rel("o", o, rows_of(ref.detach(), 49), tol), pad_ok("o", obuf, C2),
            Rel("dq", dq, rows_of(qr.grad, 49), 2 * tol), pad_ok("dq", dqbuf, C2),
            Rel("dk", dk, rows_of(kr.grad, N), 2 * tol), pad_ok("dk", dkbuf, C2),
            Rel("dv", dv, rows_of(vr.grad, N), 2 * tol), pad_ok("dv", dvbuf, C2)]

    SPLIT[cid] = (fwd, bwd)
    return Case(cid, "attention", fwd | bwd, run)


def attn_cases():
    out = []
    # N = 20: below one 32-key block; 300: two blocks of four 64-key waves, the last with 44 keys in its
    # first wave and three empty waves; 2125: 128 keys per wave, 17 chunks in 5 blocks, ragged
    for dt in (BF16, F16):
        for dh in (16, 32, 48):
            for N in (20, 300, 2125):
                out.append(attn_case(dt, N, dh))
        # zero-padded heads: below 16, between 17 and 31, the model's 36, and head dims that are no
        # multiple of 4 (the scalar repack)
        for dh, N in ((12, 300), (20, 300), (36, 2125), (10, 300), (22, 20)):
            out.append(attn_case(dt, N, dh))
        # the scalar kernels in 16-bit: head dim 64, and rows that are not 16-byte aligned
        out.append(attn_case(dt, 300, 64))
        out.append(attn_case(dt, 150, 32, aligned=False))
    out.append(attn_case(F32, 300, 32))
    out.append(attn_case(F32, 20, 12))
    return out


# ================================================================================ depthwise convolution
def _dw_apply(x4, w, k, flip=False):
    """sum_{a,j} w[c,a,j] x[b, h+a-r, w+j-r, c] (cross-correlation; flip: the input gradient's taps)."""
    r = k // 2
    B, H, W, C = x4.shape
    p = F.pad(x4, (0, 0, r, r, r, r))
    y = torch.zeros_like(x4)
    for a in range(k):
        for j in range(k):
            wt = w[:, k - 1 - a, k - 1 - j] if flip else w[:, a, j]
            y += p[:, a:a + H, j:j + W, :] * wt
    return y


def _dw_wgrad(x4, dy4, k):
    """dw[c,a,j] = sum dy[b,h,w,c] x[b,h+a-r,w+j-r,c]."""
    r = k // 2
    B, H, W, C = x4.shape
    p = F.pad(x4, (0, 0, r, r, r, r))
    dw = torch.zeros(C, k, k, dtype=x4.dtype, device=x4.device)
    for a in range(k):
        for j in range(k):
            dw[:, a, j] = (p[:, a:a + H, j:j + W, :] * dy4).sum((0, 1, 2))
    return dw


def dw_fwd_names(dt, k, H, W, C, flip, buf=True):
    t, fl = TN[dt], "true" if flip else "false"
    if k == 3 and H * W <= 65536:
        return f"dw3_stream_fwd_kernel<{t}, {fl}, {'true' if buf else 'false'}>"
    G = C // (4 if dt == F32 else 8)
    NG = 8 if G >= 8 else (4 if G >= 4 else (2 if G >= 2 else 1))
    return f"dw_tile_fwd_kernel<{t}, {k}, {fl}, {NG}, 0>"


def dw_fwd_case(dt, k, B, H, W, C, flip, far=False, tag=""):
    """Forward (dfm_dwconv_fwd, with bias and, for 3x3, the identity) or input gradient (flip:
    dfm_dwconv_bwd_data, accumulating). far: the operand is a column slice of rows so far apart that it
    spans more than 2 GiB (the pointer-addressed twin of the buffer-addressed streaming kernel)."""
    name = dw_fwd_names(dt, k, H, W, C, flip, buf=not far)
    cid = f"dw{k}-{'bwddata' if flip else 'fwd'}-{SHORT[dt]}-{B}x{H}x{W}x{C}{tag}"

    def run():
        g, kk = gen(cid), K()
        rows = B * H * W
        rdev = DEV if rows * C > BIG else "cpu"
        es = 4 if dt == F32 else 2
        x0 = rnd(g, (rows, C), dt)
        w = torch.randn(C, k, k, generator=g) * 0.3
        bias = torch.randn(C, generator=g)
        ident = k == 3
        if far:
            ldx = -(-((1 << 31) // es) // (rows - 1)) // 16 * 16 + 16
            assert ((rows - 1) * ldx + C) * es >= (1 << 31) - (1 << 20)
            big = torch.empty(rows, ldx, dtype=dt, device=DEV)  # uninitialised: only the slice is read
            x = big[:, :C]
            x.copy_(x0.to(DEV))
        else:
            x, _ = strided(x0, up8(C) + 8)
        base0 = rnd(g, (rows, C), dt)
        out, obuf = strided(base0, up8(C) + 8)
        x4, w64 = d64(x0, rdev).view(B, H, W, C), d64(w, rdev)
        with kv.Trace() as tr:
            if flip:
                kk.dwconv_bwd_data(x, (B, H, W), w.to(DEV), k, add_identity=ident, dx=out, accumulate=True)
            else:
                kk.dwconv(x, (B, H, W), w.to(DEV), bias.to(DEV), k, add_identity=ident, out=out)
        ref, S = _dw_apply(x4, w64, k, flip), _dw_apply(x4.abs(), w64.abs(), k, flip)
        if ident:
            ref, S = ref + x4, S + x4.abs()
        if flip:
            b4 = d64(base0, rdev).view(B, H, W, C)
            ref, S = ref + b4, S + b4.abs()
        else:
            ref, S = ref + d64(bias, rdev), S + d64(bias, rdev).abs()
        return tr.names, [Lin("y", out, ref.reshape(rows, C), S.reshape(rows, C), k * k + 2, U_OUT[dt]),
                          pad_ok("y", obuf, C)]

    return Case(cid, "dwconv", frozenset([name]), run)


def dw_bwd_case(dt, k, B, H, W, C, fused):
    """dfm_dwconv_bwd (input + weight + bias gradient in one pass) or dfm_dwconv_bwd_weight alone."""
    t = TN[dt]
    if fused:
        rows_ok = C % 128 == 0 or (C % 2 == 0 and C >= 384)
        name = f"dw7_bwd_fused_kernel<{t}>" if k == 7 else (
            f"dw3_rows_bwd_kernel<{t}>" if rows_ok else f"dw3_stream_bwd_kernel<{t}>")
    else:
        name = f"dw7_lds_wgrad_kernel<{t}>" if k == 7 else f"dw3_stream_wgrad_kernel<{t}>"
    cid = f"dw{k}-{'bwd' if fused else 'wgrad'}-{SHORT[dt]}-{B}x{H}x{W}x{C}"

    def run():
        g, kk = gen(cid), K()
        rows = B * H * W
        x0, dy0, base0 = rnd(g, (rows, C), dt), rnd(g, (rows, C), dt), rnd(g, (rows, C), dt)
        w = torch.randn(C, k, k, generator=g) * 0.3
        ldp = up8(C) + 8
        x, _ = strided(x0, ldp)
        dy, _ = strided(dy0, ldp)
        dx, dxbuf = strided(base0, ldp)
        ident = k == 3
        with kv.Trace() as tr:
            if fused:
                _, dw, db = kk.dwconv_bwd(x, dy, (B, H, W), w.to(DEV), k, add_identity=ident, dx=dx, accumulate=True)
            else:
                dw, db = kk.dwconv_bwd_weight(x, dy, (B, H, W), k)
        x4, dy4, w64 = d64(x0).view(B, H, W, C), d64(dy0).view(B, H, W, C), d64(w)
        checks = [Lin("dw", dw.view(C, k, k), _dw_wgrad(x4, dy4, k), _dw_wgrad(x4.abs(), dy4.abs(), k), rows,
                      U_OUT[F32]),
                  Lin("db", db, dy4.sum((0, 1, 2)), dy4.abs().sum((0, 1, 2)), rows, U_OUT[F32])]
        if fused:
            b4 = d64(base0).view(B, H, W, C)
            ref, S = _dw_apply(dy4, w64, k, True) + b4, _dw_apply(dy4.abs(), w64.abs(), k, True) + b4.abs()
            if ident:
                ref, S = ref + dy4, S + dy4.abs()
            checks += [Lin("dx", dx, ref.reshape(rows, C), S.reshape(rows, C), k * k + 2, U_OUT[dt]),
                       pad_ok("dx", dxbuf, C)]
        return tr.names, checks

    return Case(cid, "dwconv", frozenset([name, PSUM[2]]), run)


def dw_cases():
    out = []
    for dt in DTYPES:
        cpt = 4 if dt == F32 else 8
        for flip in (False, True):
            # streaming 3x3 (planes up to 65,536 pixels): two images, ragged strips and chunks
            out.append(dw_fwd_case(dt, 3, 2, 19, 37, 5 * cpt, flip))
            out.append(dw_fwd_case(dt, 3, 2, 9, 11, 2 * cpt, flip, far=True, tag="-far"))
            # LDS-tiled kernels, NG = 1 / 2 / 4 / 8 channel groups per block: G = 1, 3, 5, 9 groups, so the
            # last block of a pixel tile has a partial set of groups. 3x3: two planes just above
            # 65,536 pixels; 7x7: every plane, a small one with ragged tiles and two images
            for G in (1, 3, 5, 9):
                out.append(dw_fwd_case(dt, 3, 2, 257, 256, G * cpt, flip))
                out.append(dw_fwd_case(dt, 7, 2, 37, 45, G * cpt, flip))
        for C in (40, 128, 392):  # streaming fused backward; row-scatter (whole / partial last 64-lane slice)
            out.append(dw_bwd_case(dt, 3, 2, 19, 37, C, True))
        out.append(dw_bwd_case(dt, 3, 2, 19, 37, 40, False))
        out.append(dw_bwd_case(dt, 7, 2, 19, 37, 40, True))
        out.append(dw_bwd_case(dt, 7, 2, 19, 37, 40, False))
    return out


# ================================================================================ beyond the four families
def ew_case(dt, op, rows=333, C=72):
    """dual_mul, residual_bwd (+ its partial_sum_kernel<0> second stage) and group_scale: products of
    exact operands, each a single kernel per dtype for 16-byte aligned rows."""
    t = TN[dt]
    names = {"dual_mul": [f"dual_mul_vec_kernel<{t}>"], "residual_bwd": [f"residual_bwd_kernel<{t}>", PSUM[0]],
             "group_scale": [f"group_scale_kernel<{t}>"]}[op]
    cid = f"{op}-{SHORT[dt]}"

    def run():
        g, k = gen(cid), K()
        ldp = up8(C) + 8
        s0, m1, m2 = rnd(g, (rows, C), dt), rnd(g, (rows, C), dt), rnd(g, (rows, C), dt)
        src, _ = strided(s0, ldp)
        a, _ = strided(m1, ldp)
        b, _ = strided(m2, ldp)
        o1, o1buf = strided(torch.zeros(rows, C, dtype=dt), ldp)
        o2, o2buf = strided(torch.zeros(rows, C, dtype=dt), ldp)
        S64, A64, B64 = d64(s0), d64(m1), d64(m2)
        u = U_OUT[dt]
        if op == "dual_mul":
            with kv.Trace() as tr:
                k.dual_mul(src, a, b, out1=o1, out2=o2)
            checks = [Lin("o1", o1, S64 * A64, (S64 * A64).abs(), 1, u), pad_ok("o1", o1buf, C),
                      Lin("o2", o2, S64 * B64, (S64 * B64).abs(), 1, u), pad_ok("o2", o2buf, C)]
        elif op == "residual_bwd":
            ls, rs = torch.randn(C, generator=g), torch.randn(-(-rows // 7), generator=g)
            with kv.Trace() as tr:
                _, dls = k.residual_bwd(src, a, ls.to(DEV), rs.to(DEV), 7, df=o1)
            rr = d64(rs).repeat_interleave(7)[:rows, None]
            ref = S64 * d64(ls) * rr
            checks = [Lin("df", o1, ref, ref.abs(), 2, u), pad_ok("df", o1buf, C),
                      Lin("dls", dls, (S64 * A64 * rr).sum(0), (S64 * A64 * rr).abs().sum(0), 3 * rows, U_OUT[F32])]
        else:
            sc = torch.randn(-(-rows // 50), C, generator=g)
            with kv.Trace() as tr:
                k.group_scale(src, sc.to(DEV), 50, out=o1)
            ref = S64 * d64(sc).repeat_interleave(50, 0)[:rows]
            checks = [Lin("y", o1, ref, ref.abs(), 1, u), pad_ok("y", o1buf, C)]
        return tr.names, checks

    return Case(cid, "elementwise", frozenset(names), run)


def ew_cases():
    return ([ew_case(dt, op) for dt in DTYPES for op in ("dual_mul", "residual_bwd")] +
            [ew_case(dt, "group_scale") for dt in (BF16, F16)])


CASES = gemm_cases() + ln_cases() + pool_bilinear_cases() + attn_cases() + dw_cases() + ew_cases()
assert len({c.id for c in CASES}) == len(CASES)


def declared():
    """Every kernel name some case pins."""
    return frozenset().union(*[c.names for c in CASES])


# ================================================================================ the test
def _check(cid, chk):
    """Worst err / bound of one check (<= 1 passes)."""
    got = chk.got.detach()
    ref = chk.ref.detach().to(got.device)
    assert got.shape == ref.shape, (cid, chk.what, got.shape, ref.shape)
    if isinstance(chk, Same):
        return 0.0 if torch.equal(got, ref) else math.inf
    got = got.double()
    assert torch.isfinite(got).all(), (cid, chk.what, "non-finite output")
    err = (got - ref).abs()
    if isinstance(chk, Rel):
        return (err.max() / ref.abs().max().clamp_min(1e-300)).item() / chk.tol
    acc = 2.0 * chk.n * 2.0 ** -24 * chk.S.to(got.device)
    bound = chk.u * ref.abs() + acc
    # The rounding of the result to the output type, named explicitly: round-to-nearest errs by up to half
    # an ulp of the value's binade, 2^(e - p) for |v| in [2^e, 2^(e+1)) and p significand bits. Relative to
    # |v| that is 2^-p at the bottom of a binade and 2^-(p+1) at its top. u_out = 2^-11 (fp16, p = 11) and
    # 2^-24 (fp32, p = 24) cover the whole binade; u_out = 2^-9 for bf16 (p = 8) is the figure at the top
    # only, and a correct kernel reaches twice that just above a power of two (measured: 1.4 to 1.96 times
    # the bound without this term on every bf16 GEMM, fp32 at 0.008, fp16 within 1). The term adds what
    # u_out |r| leaves out of the half ulp (nothing for fp16 and fp32 above their subnormal range); the
    # binade is that of |r| plus the accumulation bound (and the check's extra term, which moves the value
    # before it is rounded as well), the largest value that can have been rounded.
    if chk.extra is not None:
        acc = acc + chk.extra.to(got.device)
        bound = bound + chk.extra.to(got.device)
    p, emin = ROUNDING[chk.u]
    e = torch.floor(torch.log2((ref.abs() + acc).clamp_min(2.0 ** emin)))
    bound = bound + (torch.exp2(e - p) - chk.u * ref.abs()).clamp_min(0.0)
    exact = bound == 0
    if (err[exact] != 0).any():
        return math.inf
    return (err[~exact] / bound[~exact]).max().item() if (~exact).any() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_variant(case):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    library, _ = kv.library_variants()
    launched, checks = case.run()
    torch.cuda.synchronize()
    if isinstance(launched, tuple):  # a forward and a backward call: each launches its own part
        for got, want in zip(launched, SPLIT[case.id]):
            assert got == want, (case.id, sorted(got), sorted(want))
        launched = launched[0] | launched[1]
    assert launched <= set(library), sorted(launched - set(library))
    assert launched == case.names, (case.id, sorted(launched), sorted(case.names))
    worst = {c.what: _check(case.id, c) for c in checks}
    print(f"VARIANT {case.family} {case.id} worst err/bound " +
          " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (case.id, bad)
