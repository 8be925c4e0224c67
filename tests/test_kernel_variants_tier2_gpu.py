"""The second tier of the kernel-variant ledger: the ConvFFN kernels (convffn.hip), the stem / downsample /
3x3 stride-1 data movement (conv.hip), elementwise.hip and the grouped GEMM launches, pinned by name as
tests/test_kernel_variants_gpu.py pins the hot-path families: every case names the kernels its call must
launch (from a Python transcription of the dispatch rule) and checks every output against fp64 of the
same operation on the same rounded operands.

Gates. Linear stages: Lin (|y - r| <= u_out |r| + 2 n 2^-24 S + the half-ulp term of _check). Data movement
(gathers of one tap, packs, casts, the BN shift row): bitwise. Nonlinear stages (LayerNorm, GELU, BN + GELU
gathers, softmax, the NMF quotients): the family's gate of test_kernels_gpu.py, against fp64. Where a stage
reads an operand that the kernel itself rounded to 16 bits the reference is computed from the kernel's
stored copy of it; where no copy is stored (the GELU output inside the fused ConvFFN forward without
save_gelu, and inside the dW2 pass) the bound carries that rounding as a named extra term (gelu_round_err).
The ConvFFN backward outputs that pass through the whole chain keep test_convffn_gpu.py's rule: error
against fp64 <= max(1.5 x the unfused op-level chain's error against fp64, the file's floor).

A composite entry point (dfm_convffn_bwd, a deferred-reduction group) declares the kernels of its families
that it pins: those must be launched, and no other instantiation of the same templates may be.
"""
import math
import re

import pytest
import torch
import torch.nn.functional as F

import kernel_variants as kv
import test_kernel_variants_gpu as t1
from test_kernel_variants_gpu import (BF16, DEV, DTYPES, F16, F32, PSUM, SENT, SHORT, TN, TOL, U_OUT, Case, K, Lin,
                                      Rel, Same, d64, gemm_route, gen, ln_geom, pad_ok, rnd, strided, up8)

pytestmark = pytest.mark.gpu

TF = {True: "true", False: "false"}
HALF = (BF16, F16)
# case id -> the template names of which the case's declared kernels must be the only instantiations launched
COMPOSITE = {}
# the half ulp of a value rounded to the type, relative to the value, at the bottom of a binade (_check)
HALF_ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24}


def template_name(name):
    return name.split("<", 1)[0]


def bits(t):
    """The tensor's bytes as integers (torch.equal on floats takes -0 == +0)."""
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(what, got, ref):
    return Same(what, bits(got), bits(ref.to(got.dtype)))


def red_geometry():
    """(blocks, rows per block at least) of the column reductions, from the build tag."""
    from dformer_amd import _lib
    m = re.search(r"red=(\d+)x(\d+)", _lib.BUILD_TAG)
    assert m, _lib.BUILD_TAG
    return int(m.group(1)), int(m.group(2))


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ================================================================================ C. elementwise.hip
def ew2d_case(dt, op, vec, acc):
    """dfm_scale_mul (0), dfm_gelu_bwd (1), dfm_relu_bwd (2). ew2d's rule: the 8-column kernel when C % 8 == 0 and
    every operand's rows are 16-byte aligned. The scalar route is driven by C = 71 (acc off) and by an odd
    leading dimension at C = 72 (acc on)."""
    t = TN[dt]
    name = f"ew2d_vec_kernel<{t}, {op}>" if vec else f"ew2d_kernel<{t}, {op}>"
    cid = f"ew2d-{('scale_mul', 'gelu_bwd', 'relu_bwd')[op]}-{SHORT[dt]}-{'vec' if vec else 'scalar'}-acc{int(acc)}"
    rows, rps = 333, 50  # rows_per_scale does not divide rows

    def run():
        g, k = gen(cid), K()
        C = 72 if (vec or acc) else 71
        ldp = up8(C) + 8 if (vec or not acc) else up8(C) + 9
        a0, b0, base0 = rnd(g, (rows, C), dt), rnd(g, (rows, C), dt), rnd(g, (rows, C), dt)
        a, _ = strided(a0, ldp)
        b, _ = strided(b0, ldp)
        out, obuf = strided(base0, ldp)
        A, Bm, base = d64(a0), d64(b0), d64(base0) if acc else torch.zeros(rows, C, dtype=torch.float64)
        if op == 0:
            cs, rs = torch.randn(C, generator=g), torch.randn(-(-rows // rps), generator=g)
            with kv.Trace() as tr:
                k.scale_mul(a, mul=b, colscale=cs.to(DEV), rowscale=rs.to(DEV), rows_per_scale=rps, alpha=0.75, out=out,
                            accumulate=acc)
            prod = 0.75 * A * Bm * d64(cs) * d64(rs).repeat_interleave(rps)[:rows, None]
            checks = [Lin("y", out, prod + base, prod.abs() + base.abs(), 5, U_OUT[dt])]
        elif op == 1:
            with kv.Trace() as tr:
                k.gelu_bwd(a, b, out=out, accumulate=acc)
            checks = [Rel("dx", out, A * gelu_grad64(Bm) + base, TOL[dt])]
        else:
            with kv.Trace() as tr:
                k.relu_bwd(a, b, out=out)
            checks = [same_bits("dx", out, torch.where(b0 > 0, a0, torch.zeros_like(a0)))]
        return tr.names, checks + [pad_ok("y", obuf, C)]

    return Case(cid, "elementwise", frozenset([name]), run)


def colred_case(dt, mode, variant, rows_kind, acc=False):
    """dfm_colsum without / with a multiplier (mode "sum" / "mul"), dfm_bn_stats ("bn"), dfm_bn_bwd_stats ("bnbwd").
    colred's rule: the vector kernel when C is a multiple of the 16-byte vector V, C / V <= 256, and the rows of
    x (and of y) are 16-byte aligned. variant: "vec"; "scalar" (C = 71); "oddld" (an odd leading dimension);
    "wide" (C / V = 257 lanes)."""
    t = TN[dt]
    V = 4 if dt == F32 else 8
    M = {"sum": 0, "mul": 0, "bn": 1, "bnbwd": 2}[mode]
    yp = mode in ("mul", "bnbwd")
    name = f"colred_vec_kernel<{t}, {M}, {TF[yp]}>" if variant == "vec" else f"colred_kernel<{t}, {M}>"
    cid = f"colred-{mode}-{SHORT[dt]}-{variant}-{rows_kind}" + ("-acc" if acc else "")

    def run():
        g, k = gen(cid), K()
        blocks, min_rows = red_geometry()
        # "tail": three reduction blocks, the last one partial
        rows = {"one": 1, "mid": 333, "tail": 2 * min_rows + 77}[rows_kind]
        assert rows_kind != "tail" or (blocks >= 3 and rows % 3 != 0)
        C = {"vec": 72, "scalar": 71, "oddld": 72, "wide": 257 * V}[variant]
        ldp = up8(C) + (9 if variant == "oddld" else 8)
        rps = max(1, rows // 3) + 1
        x0, y0 = rnd(g, (rows, C), dt, 3.0, 1.0), rnd(g, (rows, C), dt)
        x, _ = strided(x0, ldp)
        y, _ = strided(y0, ldp)
        X, Y = d64(x0), d64(y0)
        f32 = U_OUT[F32]
        if M == 0:
            rs = torch.randn(-(-rows // rps), generator=g)
            base0 = torch.randn(C, generator=g)
            out = base0.to(DEV)
            with kv.Trace() as tr:
                k.colsum(x, mul=y if yp else None, rowscale=rs.to(DEV), rows_per_scale=rps, out=out, accumulate=acc)
            terms = X * (Y if yp else 1.0) * d64(rs).repeat_interleave(rps)[:rows, None]
            base = d64(base0) if acc else torch.zeros(C, dtype=torch.float64)
            checks = [Lin("sum", out, terms.sum(0) + base, terms.abs().sum(0) + base.abs(), 3 * rows + 4, f32)]
        elif M == 1:
            with kv.Trace() as tr:
                st = k.bn_stats(x)
            sh = X - X[0]
            checks = [Lin("sum (x-K)", st[0], sh.sum(0), sh.abs().sum(0), rows + 4, f32),
                      Lin("sum (x-K)^2", st[1], (sh * sh).sum(0), (sh * sh).sum(0), rows + 5, f32),
                      same_bits("K", st[2], x0[0].float())]
        else:
            mean, rstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
            with kv.Trace() as tr:
                s2 = k.bn_bwd_stats(x, y, mean.to(DEV), rstd.to(DEV))
            tm = Y * (X - d64(mean)) * d64(rstd)
            checks = [Lin("sum dy", s2[0], Y.sum(0), Y.abs().sum(0), rows + 4, f32),
                      Lin("sum dy xhat", s2[1], tm.sum(0), tm.abs().sum(0), rows + 7, f32)]
        return tr.names, checks

    return Case(cid, "elementwise", frozenset([name, PSUM[0]]), run)


def bn_apply_case(dt, vec, full):
    """dfm_bn_apply: y = (x - mean) rstd gamma + beta (+ res, ReLU with `full`)."""
    t = TN[dt]
    name = f"bn_apply_vec_kernel<{t}>" if vec else f"bn_apply_kernel<{t}>"
    cid = f"bn_apply-{SHORT[dt]}-{'vec' if vec else 'scalar'}-{'res-relu' if full else 'plain'}"

    def run():
        g, k = gen(cid), K()
        rows, C = 333, 72 if vec else 71
        ldp = up8(C) + 8
        x0, r0 = rnd(g, (rows, C), dt, 2.0, 0.5), rnd(g, (rows, C), dt)
        mean, rstd, gam, bet = (torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5,
                                torch.randn(C, generator=g), torch.randn(C, generator=g))
        x, _ = strided(x0, ldp)
        res, _ = strided(r0, ldp)
        y, ybuf = strided(torch.zeros(rows, C, dtype=dt), ldp)
        with kv.Trace() as tr:
            k.bn_apply(x, mean.to(DEV), rstd.to(DEV), gam.to(DEV), bet.to(DEV), res=res if full else None,
                       act=2 if full else 0, out=y)
        ref = (d64(x0) - d64(mean)) * d64(rstd) * d64(gam) + d64(bet)
        S = (d64(x0) - d64(mean)).abs() * d64(rstd) * d64(gam).abs() + d64(bet).abs()
        if full:  # ReLU is 1-Lipschitz: the pre-activation bound holds after it
            ref, S = (ref + d64(r0)).clamp_min(0.0), S + d64(r0).abs()
        return tr.names, [Lin("y", y, ref, S, 6, U_OUT[dt]), pad_ok("y", ybuf, C)]

    return Case(cid, "elementwise", frozenset([name]), run)


def bn_bwd_apply_case(dt, vec, acc):
    """dfm_bn_bwd_apply: dx (+)= gamma rstd (dy - s0 / n - xhat s1 / n)."""
    t = TN[dt]
    name = f"bn_bwd_apply_vec_kernel<{t}>" if vec else f"bn_bwd_apply_kernel<{t}>"
    cid = f"bn_bwd_apply-{SHORT[dt]}-{'vec' if vec else 'scalar'}-acc{int(acc)}"

    def run():
        g, k = gen(cid), K()
        rows, C, count = 333, 72 if vec else 71, 333.0
        ldp = up8(C) + 8
        x0, dy0, base0 = rnd(g, (rows, C), dt, 2.0, 0.5), rnd(g, (rows, C), dt), rnd(g, (rows, C), dt)
        mean, rstd, gam = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        st = torch.randn(2, C, generator=g) * 20
        x, _ = strided(x0, ldp)
        dy, _ = strided(dy0, ldp)
        dx, dxbuf = strided(base0, ldp)
        with kv.Trace() as tr:
            k.bn_bwd_apply(x, dy, mean.to(DEV), rstd.to(DEV), gam.to(DEV), st.to(DEV), count, dx=dx, accumulate=acc)
        xh = (d64(x0) - d64(mean)) * d64(rstd)
        s = d64(gam) * d64(rstd)
        ref = s * (d64(dy0) - d64(st[0]) / count - xh * d64(st[1]) / count)
        S = s.abs() * (d64(dy0).abs() + d64(st[0]).abs() / count + xh.abs() * d64(st[1]).abs() / count)
        if acc:
            ref, S = ref + d64(base0), S + d64(base0).abs()
        return tr.names, [Lin("dx", dx, ref, S, 10, U_OUT[dt]), pad_ok("dx", dxbuf, C)]

    return Case(cid, "elementwise", frozenset([name]), run)


def bn_finalize_case(C, running):
    cid = f"bn_finalize-c{C}-{'running' if running else 'plain'}"

    def run():
        g, k = gen(cid), K()
        count, eps, mom = 1234.0, 1e-3, 0.1
        st = torch.stack([torch.randn(C, generator=g) * count * 0.1, (torch.rand(C, generator=g) + 0.5) * count,
                          torch.randn(C, generator=g) * 3])
        rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        rm, rv = (rm0.to(DEV), rv0.to(DEV)) if running else (None, None)
        with kv.Trace() as tr:
            mean, rstd = k.bn_finalize(st.to(DEV), count, eps, mom, rm, rv)
        s = d64(st)
        d = s[0] / count
        mu, var = s[2] + d, s[1] / count - d * d
        tol = TOL[F32]
        checks = [Rel("mean", mean, mu, tol), Rel("rstd", rstd, 1.0 / (var + eps).sqrt(), tol)]
        if running:
            checks += [Rel("running_mean", rm, (1 - mom) * d64(rm0) + mom * mu, tol),
                       Rel("running_var", rv, (1 - mom) * d64(rv0) + mom * var * count / (count - 1.0), tol)]
        return tr.names, checks

    return Case(cid, "elementwise", frozenset(["bn_finalize_kernel"]), run)


def bn_merge_case(shards, C):
    cid = f"bn_merge-s{shards}-c{C}"

    def run():
        g, k = gen(cid), K()
        counts = torch.tensor([100.0, 333.0, 57.0][:shards])
        parts = torch.stack([torch.stack([torch.randn(C, generator=g) * n * 0.1, (torch.rand(C, generator=g) + 0.5) * n,
                                          torch.randn(C, generator=g) * 3]) for n in counts.tolist()])
        with kv.Trace() as tr:
            st = k.bn_merge(parts.to(DEV), counts.to(DEV))
        if shards == 1:  # the identity, bit for bit
            return tr.names, [same_bits("stats", st, parts[0])]
        p, n = d64(parts), d64(counts)[:, None]
        dd = p[:, 2] - p[0, 2]
        s1 = (p[:, 0] + n * dd).sum(0)
        s2 = (p[:, 1] + 2.0 * dd * p[:, 0] + n * dd * dd).sum(0)
        return tr.names, [Rel("S1", st[0], s1, TOL[F32]), Rel("S2", st[1], s2, TOL[F32]),
                          same_bits("K", st[2], parts[0, 2])]

    return Case(cid, "elementwise", frozenset(["bn_merge_kernel"]), run)


def _cast_source(g, dt):
    """Every value a cast can get wrong: for a 16-bit source all 65,536 bit patterns (NaNs replaced); for fp32
    ties of round-to-nearest-even in both 16-bit types, +-0, +-inf, the targets' subnormals and their ties,
    fp16 / bf16 overflow to inf and its tie, an fp32 subnormal, and 1,000 normal values."""
    if dt != F32:
        v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)
        return torch.where(torch.isnan(v), torch.zeros_like(v), v)
    p = lambda e: 2.0 ** e  # noqa: E731
    special = [0.0, -0.0, math.inf, -math.inf, 1.0, 1 + p(-8), 1 + 3 * p(-8), -(1 + p(-8)), 1 + p(-8) + p(-20),
               1 + p(-11), 1 + 3 * p(-11), 1 + p(-11) - p(-23), 65504.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e5,
               3.3895313892515355e38, 3.3961775292304e38, 3.4e38, -3.4e38, p(-14), p(-24), p(-25), 3 * p(-25),
               p(-25) + p(-40), p(-26), p(-126), p(-127), p(-133), p(-134), 3 * p(-134), p(-135), p(-149)]
    return torch.cat([torch.tensor(special, dtype=torch.float32), torch.randn(1000, generator=g) * 50])


def cast_case(di, do):
    cid = f"cast-{SHORT[di]}-{SHORT[do]}"

    def run():
        g, k = gen(cid), K()
        x0 = _cast_source(g, di)
        assert x0.numel() % 256 != 0 or di != F32
        guard = torch.full((x0.numel() + 64,), SENT, dtype=do, device=DEV)
        out = guard[:x0.numel()]
        with kv.Trace() as tr:
            k.cast(x0.to(DEV), do, out=out)
        return tr.names, [same_bits("y", out, x0.to(do)),
                          Same("y tail", guard[x0.numel():], torch.full((64,), SENT, dtype=do, device=DEV))]

    return Case(cid, "elementwise", frozenset([f"cast_kernel<{TN[di]}, {TN[do]}>"]), run)


def pack_case(do, cols):
    """dfm_pack_slices: the 8-column kernel for a 16-bit output with cols % 8 == 0 (and aligned operands)."""
    vec = do != F32 and cols % 8 == 0
    name = f"pack_slices_vec_kernel<{TN[do]}>" if vec else f"pack_slices_kernel<{TN[do]}>"
    cid = f"pack_slices-{SHORT[do]}-cols{cols}"

    def run():
        g, k = gen(cid), K()
        rows = 333
        srcs = [rnd(g, (rows, cols), dt, 30.0) for dt in (F32, BF16, F16, F32)]
        out = torch.full((rows, 4 * cols), SENT, dtype=do, device=DEV)
        with kv.Trace() as tr:
            k.pack_slices([s.to(DEV) for s in srcs], out)
        return tr.names, [same_bits("packed", out, torch.cat([s.float().to(do) for s in srcs], 1))]

    return Case(cid, "elementwise", frozenset([name]), run)


def nonfinite_case(kind):
    cid = f"nonfinite-{kind}"

    def run():
        g, k = gen(cid), K()
        n = 100001  # no multiple of the block
        x = torch.randn(n, generator=g)
        if kind == "inf-first":
            x[0] = math.inf
        elif kind == "nan-last":
            x[-1] = math.nan
        elif kind == "neginf-mid":
            x[n // 2 + 13] = -math.inf
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        with kv.Trace() as tr:
            k.grad_nonfinite(x.to(DEV), flag)
        return tr.names, [Same("flag", flag, torch.tensor([0 if kind == "clean" else 1], dtype=torch.int32))]

    return Case(cid, "elementwise", frozenset(["nonfinite_kernel"]), run)


def psum_group_case(dt):
    """Three deferred second stages in one dfm_partial_sum_group launch, one per output layout: the
    layer-scale gradient (one vector), LayerNorm dgamma / dbeta (two vectors), the depthwise weight / bias
    gradient (interleaved)."""
    t = TN[dt]
    C, B, H, W = 72, 2, 9, 11
    geom = ln_geom(dt, C)
    ln = f"ln_bwd_vec_kernel<{t}, {geom[1]}, {geom[2]}>" if geom[0] == "vec" else f"ln_bwd_kernel<{t}, {geom[1]}>"
    names = frozenset([f"residual_bwd_kernel<{t}>", ln, f"dw3_stream_bwd_kernel<{t}>", "partial_sum_group_kernel"])
    cid = f"psum_group-{SHORT[dt]}"

    def run():
        g, k = gen(cid), K()
        rows = B * H * W
        x0, dy0, f0 = rnd(g, (rows, C), dt, 2.0, 0.5), rnd(g, (rows, C), dt), rnd(g, (rows, C), dt)
        gam, bet, ls, rs = (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g),
                            torch.randn(B, generator=g))
        w = torch.randn(C, 3, 3, generator=g) * 0.3
        x, dy, f = x0.to(DEV), dy0.to(DEV), f0.to(DEV)
        _, mean, rstd = k.layernorm(x, gam.to(DEV), bet.to(DEV), 1e-6)
        with kv.Trace() as tr:
            with k.wgrad_group():
                _, dls = k.residual_bwd(dy, f, ls.to(DEV), rs.to(DEV), H * W)
                _, dg, db = k.layernorm_bwd(x, dy, gam.to(DEV), mean, rstd)
                _, dw, dwb = k.dwconv_bwd(x, dy, (B, H, W), w.to(DEV), 3, add_identity=True)
        xr, gr, br = d64(x0).requires_grad_(), d64(gam).requires_grad_(), d64(bet).requires_grad_()
        F.layer_norm(xr, (C,), gr, br, 1e-6).backward(d64(dy0))
        rr = d64(rs).repeat_interleave(H * W)[:, None]
        tl = d64(dy0) * d64(f0) * rr
        x4, dy4 = d64(x0).view(B, H, W, C), d64(dy0).view(B, H, W, C)
        tol = TOL[dt]
        return tr.names, [
            Lin("dls", dls, tl.sum(0), tl.abs().sum(0), 3 * rows, U_OUT[F32]),
            Rel("dgamma", dg, gr.grad, 2 * tol), Rel("dbeta", db, br.grad, tol),
            Lin("dw", dw.view(C, 3, 3), t1._dw_wgrad(x4, dy4, 3), t1._dw_wgrad(x4.abs(), dy4.abs(), 3), rows,
                U_OUT[F32]),
            Lin("db", dwb, dy4.sum((0, 1, 2)), dy4.abs().sum((0, 1, 2)), rows, U_OUT[F32])]

    COMPOSITE[cid] = True
    return Case(cid, "elementwise", names, run)


def psum_group_chunks_case():
    """17 deferred reductions: dfm_partial_sum_group issues them as two launches (16 per launch)."""
    cid = "psum_group-17-sums"
    names = frozenset(["residual_bwd_kernel<float>", "partial_sum_group_kernel"])

    def run():
        g, k = gen(cid), K()
        rows, C = 130, 72
        ops = [(rnd(g, (rows, C), F32), rnd(g, (rows, C), F32), torch.randn(C, generator=g)) for _ in range(17)]
        dev = [(a.to(DEV), b.to(DEV), c.to(DEV)) for a, b, c in ops]
        with kv.Trace() as tr:
            with k.wgrad_group():
                outs = [k.residual_bwd(a, b, c)[1] for a, b, c in dev]
        nl = torch.tensor([tr.launched.count("partial_sum_group_kernel")])
        checks = [Same("second-stage launches", nl, torch.tensor([2]))]
        for i, ((a, b, _), o) in enumerate(zip(ops, outs)):
            tm = d64(a) * d64(b)
            checks.append(Lin(f"dls{i}", o, tm.sum(0), tm.abs().sum(0), 3 * rows, U_OUT[F32]))
        return tr.names, checks

    return Case(cid, "elementwise", names, run)


def softmax_case(R, acc):
    """dfm_softmax_rows / _bwd, one wave per row (gate of test_nmf_update_softmax, against fp64)."""
    cid = f"softmax_rows-r{R}-acc{int(acc)}"
    names = ("softmax_rows_kernel", "softmax_rows_bwd_kernel")

    def run():
        g, k = gen(cid), K()
        rows = 333  # no multiple of the 4 rows of a block
        x0, gy0, base0 = torch.randn(rows, R, generator=g) * 3, torch.randn(rows, R, generator=g), \
            torch.randn(rows, R, generator=g)
        with kv.Trace() as ta:
            y = k.softmax_rows(x0.to(DEV))
        dx = base0.to(DEV)
        with kv.Trace() as tb:
            k.softmax_rows_bwd(y, gy0.to(DEV), dx=dx, accumulate=acc)
        yr = d64(x0).softmax(-1)
        ys = d64(y.cpu())  # the backward is checked from the forward's stored output
        ref = ys * (d64(gy0) - (ys * d64(gy0)).sum(-1, keepdim=True)) + (d64(base0) if acc else 0.0)
        return (ta.names, tb.names), [Rel("y", y, yr, 1e-5), Rel("dx", dx, ref, 1e-5)]

    t1.SPLIT[cid] = (frozenset(names[:1]), frozenset(names[1:]))
    return Case(cid, "elementwise", frozenset(names), run)


def nmf_case(cdt, fused):
    """The NMF multiplicative update and its backward, elementwise (dfm_nmf_update / _bwd) or with the rank-64
    denominator products fused (dfm_nmf_update_mm / _bwd_mm), with a 16-bit copy of the result in `cdt`. Gates
    of test_nmf_update_softmax / test_nmf_update_mm_fused, against fp64; the copy is the stored result's cast."""
    t = TN[cdt]
    fwd, bwd = (f"nmf_update_mm_kernel<{t}>", f"nmf_update_bwd_mm_kernel<{t}>") if fused else \
        (f"nmf_update_kernel<{t}>", f"nmf_update_bwd_kernel<{t}>")
    cid = f"nmf_update{'_mm' if fused else ''}-{SHORT[cdt]}"

    def run():
        g, k = gen(cid), K()
        Bb, rows, R, eps = 3, 77, 64, 1e-6  # 77 rows: two 64-row blocks per batch, the second partial
        a0, num0 = torch.rand(Bb, rows, R, generator=g) + 0.1, torch.rand(Bb, rows, R, generator=g)
        g0 = torch.randn(Bb, rows, R, generator=g)
        a, num, gg = a0.to(DEV), num0.to(DEV), g0.to(DEV)
        A, N, G = d64(a0), d64(num0), d64(g0)
        if not fused:
            den0, base0 = torch.rand(Bb, rows, R, generator=g) + 0.1, torch.randn(Bb, rows, R, generator=g)
            den, ga = den0.to(DEV), base0.to(DEV)
            with kv.Trace() as ta:
                out, o16 = k.nmf_update(a, num, den, eps, bf16_copy=cdt)
            with kv.Trace() as tb:
                _, gnum, gden, g16 = k.nmf_update_bwd(gg, a, num, den, out, ga=ga, accumulate=True, eps=eps,
                                                      bf16_copy=cdt)
            D, O = d64(den0), d64(out.cpu())
            r = 1.0 / (D + eps)
            checks = [Rel("out", out, A * N * r, 1e-6), same_bits("out16", o16, out.to(cdt)),
                      Rel("ga", ga, d64(base0) + G * N * r, 1e-5), Rel("gnum", gnum, G * A * r, 1e-5),
                      Rel("gden", gden, -G * O * r, 1e-5), same_bits("gnum16", g16, gnum.to(cdt))]
            return (ta.names, tb.names), checks
        Bm = torch.rand(Bb, 96, R, generator=g)
        M0 = (Bm.transpose(1, 2) @ Bm)
        A20, S0 = torch.rand(Bb, rows, R, generator=g), torch.randn(Bb, R, R, generator=g)
        Md = M0.to(DEV)
        with kv.Trace() as ta:
            out, den, o16 = k.nmf_update_mm(a, num, Md, eps, bf16_copy=cdt)
        with kv.Trace() as tb:
            ga, gnum, gden, g16 = k.nmf_update_bwd_mm(gg, a, num, den, out, A2=A20.to(DEV), S=S0.to(DEV), Mg=Md,
                                                      eps=eps, bf16_copy=cdt)
        M64 = d64(M0)
        Dk, O = d64(den.cpu()), d64(out.cpu())  # the later stages are checked from the stored den / out
        ge = G + d64(A20) @ (d64(S0) + d64(S0).transpose(1, 2))
        r = 1.0 / (Dk + eps)
        gden_ref = -ge * O * r
        checks = [Rel("den", den, A @ M64, 1e-5), Rel("out", out, A * N / (Dk + eps), 1e-5),
                  same_bits("out16", o16, out.to(cdt)), Rel("gnum", gnum, ge * A * r, 1e-5),
                  Rel("gden", gden, gden_ref, 1e-5), Rel("ga", ga, ge * N * r + gden_ref @ M64, 1e-5),
                  same_bits("gnum16", g16, gnum.to(cdt))]
        return (ta.names, tb.names), checks

    t1.SPLIT[cid] = (frozenset([fwd]), frozenset([bwd]))
    return Case(cid, "elementwise", frozenset([fwd, bwd]), run)


def elementwise_cases():
    out = []
    for dt in DTYPES:
        for op in (0, 1, 2):
            for vec in (True, False):
                for acc in ((False,) if op == 2 else (False, True)):
                    out.append(ew2d_case(dt, op, vec, acc))
        for mode in ("sum", "mul", "bn", "bnbwd"):
            acc = mode in ("sum", "mul")
            out += [colred_case(dt, mode, "vec", "one"), colred_case(dt, mode, "vec", "mid", acc),
                    colred_case(dt, mode, "vec", "tail"), colred_case(dt, mode, "scalar", "mid"),
                    colred_case(dt, mode, "oddld", "tail", acc), colred_case(dt, mode, "wide", "mid")]
        for vec in (True, False):
            for flag in (False, True):
                out.append(bn_apply_case(dt, vec, flag))
                out.append(bn_bwd_apply_case(dt, vec, flag))
        out.append(psum_group_case(dt))
    out += [bn_finalize_case(300, True), bn_finalize_case(71, False), bn_merge_case(3, 300), bn_merge_case(1, 71)]
    out += [cast_case(a, b) for a, b in ((F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32),
                                         (F16, F16))]
    out += [pack_case(F32, 8), pack_case(BF16, 8), pack_case(F16, 8), pack_case(BF16, 7), pack_case(F16, 7)]
    out += [nonfinite_case(kd) for kd in ("clean", "inf-first", "nan-last", "neginf-mid")]
    out += [psum_group_chunks_case(), softmax_case(64, False), softmax_case(100, True)]
    out += [nmf_case(cdt, fused) for cdt in HALF for fused in (False, True)]
    return out


# ================================================================================ D. grouped GEMM
def group_splits(members):
    """group_splits: split-K slices in proportion to a problem's share of the group's tiles x K, a forced
    count where split_k >= 1."""
    work = sum(-(-m["M"] // 128) * -(-(m["N"] + bool(m.get("colsum"))) // 128) * m["K"] for m in members)
    per_blk = max(512.0, work / 512.0)
    out = []
    for m in members:
        if m.get("split_k", 0) >= 1:
            out.append(m["split_k"])
            continue
        p2 = 1
        while 2.0 * p2 <= m["K"] / per_blk and p2 < 256:
            p2 *= 2
        out.append(p2)
    return out


def group_route(dt, ak, bk, members):
    """gemm_group_typed: a k-contiguous-A group runs its ring members (16-bit, aligned, K >= 128, unsplit, no
    bias-gradient column) as one gemm_glds_group_kernel launch (a single ring member and every other member
    on dfm_gemm's own route); any other group is one gemm_group_kernel launch plus one combine when a member
    is split."""
    t = TN[dt]
    if not ak:
        names = [f"gemm_group_kernel<{t}, 128, 128, 8, 2, {32 if dt == F32 else 64}, false, {TF[bk]}, 2>"]
        if any(s > 1 for s in group_splits(members)):
            names.append(f"splitk_reduce_group_kernel<{t}>")
        return names
    ring, names = [], []
    for m in members:
        if dt != F32 and m["aligned"] and m["K"] >= 128 and m.get("split_k", 0) <= 1 and not m.get("colsum"):
            ring.append(m)
        else:
            names += gemm_route(dt, m["M"], m["N"], m["K"], True, bk, m["aligned"], m.get("split_k", 0))
    if len(ring) == 1:
        m = ring[0]
        names += gemm_route(dt, m["M"], m["N"], m["K"], True, bk, True, m.get("split_k", 0))
    elif ring:
        names.append(f"gemm_glds_group_kernel<{t}, 64, 64, 4, 2, true, {TF[bk]}, 2, 4>")
    return names


def group_case(cid, dt, ak, bk, members):
    """One dfm_gemm_group call. A member: M, N, K, aligned (leading dimensions multiples of 8, else odd),
    split_k, beta, bias, colsum (the bias-gradient column: row sums of A), f32 (fp32 output of 16-bit operands)."""
    names = frozenset(group_route(dt, ak, bk, members))
    splits = group_splits(members)

    def run():
        g, k = gen(cid), K()
        items, checks, keep = [], [], []
        for i, m in enumerate(members):
            M, N, Kd = m["M"], m["N"], m["K"]
            pad = (lambda c: up8(c) + 8) if m["aligned"] else (lambda c: up8(c) + 1)
            odt = F32 if m.get("f32") else dt
            a0 = rnd(g, (M, Kd) if ak else (Kd, M), dt)
            b0 = rnd(g, (N, Kd) if bk else (Kd, N), dt)
            c0 = rnd(g, (M, N), odt)
            a, _ = strided(a0, pad(a0.shape[1]))
            b, _ = strided(b0, pad(b0.shape[1]))
            out, obuf = strided(c0, pad(N))
            bias = torch.randn(N, generator=g) if m.get("bias") else None
            cs = torch.full((M + 8,), SENT, dtype=torch.float32, device=DEV) if m.get("colsum") else None
            beta = float(m.get("beta", 0.0))
            k.gemm(a, b, M=M, N=N, K=Kd, a_kcontig=ak, b_kcontig=bk, lda=a.stride(0), ldb=b.stride(0), out=out,
                   ldc=out.stride(0), beta=beta, bias=bias.to(DEV) if bias is not None else None,
                   split_k=m.get("split_k", 0), colsum=cs[:M] if cs is not None else None, collect=items)
            A = d64(a0) if ak else d64(a0).t()
            Bm = d64(b0).t() if bk else d64(b0)
            ref, S = A @ Bm, A.abs() @ Bm.abs()
            if bias is not None:
                ref, S = ref + d64(bias), S + d64(bias).abs()
            if beta:
                ref, S = ref + d64(c0), S + d64(c0).abs()
            n = Kd + 2 + (splits[i] if not ak else 0)
            checks += [Lin(f"y{i}", out, ref, S, n, U_OUT[odt]), pad_ok(f"y{i}", obuf, N)]
            if cs is not None:
                checks += [Lin(f"colsum{i}", cs[:M], A.sum(1), A.abs().sum(1), n, U_OUT[F32]),
                           Same(f"colsum{i} tail", cs[M:], torch.full((8,), SENT, device=DEV))]
            keep.append((a, b, out, bias, cs))
        with kv.Trace() as tr:
            k._launch_gemm_group(items)
        return tr.names, checks

    return Case(cid, "gemm", names, run)


def group_cases():
    out = []
    # weight-gradient layout (row-contiguous A), three members of different M and N in one launch: a
    # bias-gradient column at N = 128 (the extra column opens a tile of its own) split in two; an unsplit
    # accumulating member in between (so the third member's workspace offset and reduction block range follow a
    # member without either); a third split in four, on odd leading dimensions
    wg = [dict(M=150, N=128, K=1100, aligned=True, split_k=2, colsum=True, f32=True),
          dict(M=70, N=40, K=200, aligned=True, beta=1.0, bias=True),
          dict(M=200, N=136, K=1100, aligned=False, split_k=4, f32=True)]
    assert group_splits(wg) == [2, 1, 4]
    for dt in DTYPES:
        for bk in (False, True):
            out.append(group_case(f"group-wgrad-{SHORT[dt]}-b{int(bk)}", dt, False, bk, wg))
        # no member split (no combine launch): the bias-gradient column written by the tile's own epilogue
        out.append(group_case(f"group-wgrad-{SHORT[dt]}-unsplit", dt, False, False,
                              wg[1:2] + [dict(wg[1], M=33, N=128, colsum=True, f32=True)]))
    # forward / input-gradient layout (k-contiguous A): two ring members (one wider than tall, one
    # accumulating) in one grouped launch, a short-K and a misaligned member on dfm_gemm's own route
    fw = [dict(M=150, N=136, K=200, aligned=True, bias=True), dict(M=50, N=136, K=328, aligned=True, beta=1.0),
          dict(M=150, N=24, K=72, aligned=True, bias=True), dict(M=150, N=56, K=200, aligned=False)]
    for dt in HALF:
        for bk in (True, False):
            out.append(group_case(f"group-kcontig-{SHORT[dt]}-b{int(bk)}", dt, True, bk, fw))
            # a single ring member is handed to dfm_gemm with the rest
            out.append(group_case(f"group-kcontig-{SHORT[dt]}-b{int(bk)}-one-ring", dt, True, bk, [fw[0], fw[2]]))
    out.append(group_case("group-kcontig-f32-b1", F32, True, True, fw[:3]))
    return out


# ================================================================================ B. conv.hip data movement
PLANES = [(1, 1), (2, 1), (5, 7), (6, 4)]  # odd and even sizes: Ho = (H + 1) / 2 both ways; B = 2 throughout
IM2COL_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F32, F16), (F16, F16)]
COL2IM_GEN_PAIRS = [(F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16), (F32, BF16)]


def _gather_s2(x4, kp):
    """cols[(b, oh, ow), (kh*3+kw)*Cin + c] = x[b, c, 2oh-1+kh, 2ow-1+kw] (0 outside, 0 past 9 Cin) of an
    NCHW tensor, in its dtype: data movement only."""
    B, C, H, W = x4.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    p = F.pad(x4, (1, 2, 1, 2))
    cols = torch.zeros(B, Ho, Wo, kp, dtype=x4.dtype)
    for kh in range(3):
        for kw in range(3):
            tap = p[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2]
            cols[..., (kh * 3 + kw) * C:(kh * 3 + kw + 1) * C] = tap.permute(0, 2, 3, 1)
    return cols.reshape(B * Ho * Wo, kp)


def _scatter_s2(dc, B, H, W, C):
    """The transpose of _gather_s2 on fp64 dcols [M, >= 9C]: dx [B, H, W, C]."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    d = dc.view(B, Ho, Wo, -1)
    p = torch.zeros(B, 2 * Ho + 2, 2 * Wo + 2, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            p[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] += d[..., (kh * 3 + kw) * C:(kh * 3 + kw + 1) * C]
    return p[:, 1:H + 1, 1:W + 1]


def im2col_case(ti, to, how, H, W, Cin, bn=False, gelu=False):
    """dfm_conv3s2_im2col. im2col_typed's rule: the vector gather when the channel stride is 1, Cin % 8 == 0,
    Kp == 9 Cin, the base is 16-byte aligned and the batch / row / pixel strides are multiples of 8; `how`
    drives one term false at a time: "nhwc" (all true for Cin % 8 == 0), "kp" (Kp = 9 Cin + 8), "nchw"
    (channel stride H W), "offset" (base 8 bytes off), "batch" (batch stride + 4 elements)."""
    B = 2
    vec = how == "nhwc" and Cin % 8 == 0
    name = f"im2col_{'vec' if vec else 'gen'}_kernel<{TN[ti]}, {TN[to]}, unsigned int>"
    cid = f"im2col-{SHORT[ti]}-{SHORT[to]}-{how}-{H}x{W}x{Cin}" + ("-bn" if bn else "") + ("-gelu" if gelu else "")

    def run():
        from dformer_amd import _lib
        g = gen(cid)
        kp = up8(9 * Cin) + (8 if how == "kp" else 0)
        x0 = rnd(g, (B, Cin, H, W), ti)  # NCHW-logical values
        off = (8 // x0.element_size()) if how == "offset" else 0
        bpad = 4 if how == "batch" else 0
        if how == "nchw":
            buf = torch.full((B * Cin * H * W,), SENT, dtype=ti, device=DEV)
            x = buf.view(B, Cin, H, W)
        else:
            buf = torch.full((off + B * (H * W * Cin + bpad),), SENT, dtype=ti, device=DEV)
            x = buf[off:].view(B, H * W * Cin + bpad)[:, :H * W * Cin].view(B, H, W, Cin).permute(0, 3, 1, 2)
        x.copy_(x0.to(DEV))
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        M = B * Ho * Wo
        guard = torch.full((M + 1, kp), SENT, dtype=to, device=DEV)
        par = [torch.randn(Cin, generator=g), torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g),
               torch.randn(Cin, generator=g)] if bn else None
        dpar = [p.to(DEV) for p in par] if bn else [None] * 4
        sb, sc, sh, sw = x.stride()
        with kv.Trace() as tr:
            _lib.check(_lib.lib.dfm_conv3s2_im2col(_lib.dtype_code(x), _lib.dtype_code(guard), B, H, W, Cin, sb, sc, sh,
                                                   sw, _lib.ptr(x), *[_lib.ptr(p) for p in dpar], int(gelu), kp,
                                                   _lib.ptr(guard), _lib.stream()), "dfm_conv3s2_im2col")
        tail = Same("row past the end", guard[M], torch.full((kp,), SENT, dtype=to, device=DEV))
        if not (bn or gelu):
            return tr.names, [same_bits("cols", guard[:M], _gather_s2(x0.float().to(to), kp)), tail]
        v = d64(x0)
        if bn:
            mean, rstd, gam, bet = (d64(p)[None, :, None, None] for p in par)
            v = (v - mean) * rstd * gam + bet
        if gelu:
            v = gelu64(v)
        # the activation applies to pixels inside the image only: outside (and past 9 Cin) the operand is 0
        ref = _gather_s2(v, kp)
        zero = _gather_s2(torch.ones_like(v), kp) == 0
        return tr.names, [Rel("cols", guard[:M], ref, TOL[to]),
                          Same("zero fill", guard[:M][zero.to(DEV)],
                               torch.zeros(int(zero.sum()), dtype=to, device=DEV)),
                          tail]

    return Case(cid, "conv", frozenset([name]), run)


def col2im_vec_case(dt, H, W, Cin, acc, act=None):
    """dfm_conv3s2_col2im: at most 4 taps reach an input pixel. act: None, "gelu" (x GELU'(x)), "bn-gelu"
    (x GELU' of the folded BatchNorm of x)."""
    B = 2
    cid = f"col2im_s2-{SHORT[dt]}-{H}x{W}x{Cin}-acc{int(acc)}" + (f"-{act}" if act else "")

    def run():
        g, k = gen(cid), K()
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        M, P = B * Ho * Wo, B * H * W
        dc0, x0, base0 = rnd(g, (M, 9 * Cin), dt), rnd(g, (P, Cin), dt), rnd(g, (P, Cin), dt)
        dc, _ = strided(dc0, 9 * Cin + 8)
        x, _ = strided(x0, Cin + 8)
        dx, dxbuf = strided(base0, Cin + 16)
        par = [torch.randn(Cin, generator=g), torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g),
               torch.randn(Cin, generator=g)]
        with kv.Trace() as tr:
            k.conv3s2_col2im(dc, (B, H, W), Cin, x=x if act else None, bn=[p.to(DEV) for p in par] if act == "bn-gelu"
                             else None, gelu=bool(act), dx=dx, accumulate=acc)
        ref = _scatter_s2(d64(dc0), B, H, W, Cin).reshape(P, Cin)
        S = _scatter_s2(d64(dc0).abs(), B, H, W, Cin).reshape(P, Cin)
        base = d64(base0) if acc else torch.zeros_like(ref)
        if act is None:
            chk = Lin("dx", dx, ref + base, S + base.abs(), 4 + 1, U_OUT[dt])
        else:
            z = d64(x0)
            if act == "bn-gelu":
                z = (z - d64(par[0])) * d64(par[1]) * d64(par[2]) + d64(par[3])
            chk = Rel("dx", dx, ref * gelu_grad64(z) + base, TOL[dt])
        return tr.names, [chk, pad_ok("dx", dxbuf, Cin)]

    return Case(cid, "conv", frozenset([f"col2im_vec_kernel<{TN[dt]}, unsigned int>"]), run)


def col2im_gen_case(ti, to, H, W, Cin):
    """dfm_conv3s2_col2im_nchw: the image's own gradient, contiguous NCHW in `to`."""
    B = 2
    cid = f"col2im_nchw-{SHORT[ti]}-{SHORT[to]}-{H}x{W}x{Cin}"

    def run():
        g, k = gen(cid), K()
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        dc0 = rnd(g, (B * Ho * Wo, 9 * Cin), ti)
        dc, _ = strided(dc0, up8(9 * Cin) + 8)
        with kv.Trace() as tr:
            dx = k.conv3s2_col2im_nchw(dc, (B, H, W), Cin, to)
        ref = _scatter_s2(d64(dc0), B, H, W, Cin).permute(0, 3, 1, 2)
        S = _scatter_s2(d64(dc0).abs(), B, H, W, Cin).permute(0, 3, 1, 2)
        return tr.names, [Lin("dx", dx, ref, S, 4, U_OUT[to])]

    return Case(cid, "conv", frozenset([f"col2im_gen_kernel<{TN[ti]}, {TN[to]}>"]), run)


def conv_s1_case(dt, H, W, Cin, acc):
    """dfm_conv3s1_im2col (bitwise) and dfm_conv3s1_col2im (up to 9 taps per pixel) on strided rows."""
    B = 2
    t = TN[dt]
    cid = f"conv3s1-{SHORT[dt]}-{H}x{W}x{Cin}-acc{int(acc)}"
    fwd, bwd = f"im2col_s1_kernel<{t}, unsigned int>", f"col2im_s1_kernel<{t}, unsigned int>"

    def run():
        g, k = gen(cid), K()
        P = B * H * W
        x0, dc0, base0 = rnd(g, (P, Cin), dt), rnd(g, (P, 9 * Cin), dt), rnd(g, (P, Cin), dt)
        x, _ = strided(x0, Cin + 8)
        cols, cbuf = strided(torch.zeros(P, 9 * Cin, dtype=dt), 9 * Cin + 8)
        dc, _ = strided(dc0, 9 * Cin + 16)
        dx, dxbuf = strided(base0, Cin + 8)
        with kv.Trace() as ta:
            k.conv3s1_im2col(x, (B, H, W), out=cols)
        with kv.Trace() as tb:
            k.conv3s1_col2im(dc, (B, H, W), Cin, dx=dx, accumulate=acc)
        x4 = x0.view(B, H, W, Cin)
        p = F.pad(x4, (0, 0, 1, 1, 1, 1))
        want = torch.cat([p[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], -1).reshape(P, 9 * Cin)
        d4 = d64(dc0).view(B, H, W, 9, Cin)

        def scatter(d):
            q = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.float64)
            for kh in range(3):
                for kw in range(3):
                    q[:, kh:kh + H, kw:kw + W] += d[:, :, :, kh * 3 + kw]
            return q[:, 1:H + 1, 1:W + 1].reshape(P, Cin)

        base = d64(base0) if acc else torch.zeros(P, Cin, dtype=torch.float64)
        return (ta.names, tb.names), [
            same_bits("cols", cols, want), pad_ok("cols", cbuf, 9 * Cin),
            Lin("dx", dx, scatter(d4) + base, scatter(d4.abs()) + base.abs(), 9 + 1, U_OUT[dt]),
            pad_ok("dx", dxbuf, Cin)]

    t1.SPLIT[cid] = (frozenset([fwd]), frozenset([bwd]))
    return Case(cid, "conv", frozenset([fwd, bwd]), run)


def weight_pack_case(dt, Cin):
    cid = f"weight_pack-{SHORT[dt]}-cin{Cin}"

    def run():
        g, k = gen(cid), K()
        cout, kp = 5, up8(9 * Cin)
        w = torch.randn(cout, Cin, 3, 3, generator=g)
        with kv.Trace() as tr:
            wp = k.conv3_weight_pack(w.to(DEV), dt, kp)
        want = torch.zeros(cout, kp, dtype=dt)
        want[:, :9 * Cin] = w.permute(0, 2, 3, 1).reshape(cout, 9 * Cin).to(dt)
        return tr.names, [same_bits("wp", wp, want)]

    return Case(cid, "conv", frozenset([f"weight_pack_kernel<{TN[dt]}>"]), run)


def weight_unpack_case(Cin, acc):
    cid = f"weight_unpack-cin{Cin}-acc{int(acc)}"

    def run():
        g, k = gen(cid), K()
        cout, kp = 5, up8(9 * Cin)
        dwp, base = torch.randn(cout, kp, generator=g), torch.randn(cout, Cin, 3, 3, generator=g)
        dw = base.to(DEV)
        with kv.Trace() as tr:
            k.conv3_weight_unpack(dwp.to(DEV), Cin, dw=dw, accumulate=acc)
        v = dwp[:, :9 * Cin].reshape(cout, 3, 3, Cin).permute(0, 3, 1, 2)
        return tr.names, [same_bits("dw", dw, base + v if acc else v)]  # one fp32 add: correctly rounded either way

    return Case(cid, "conv", frozenset(["weight_unpack_kernel"]), run)


def conv_cases():
    out = []
    for ti, to in IM2COL_PAIRS:
        for H, W in PLANES:
            out.append(im2col_case(ti, to, "nhwc", H, W, 16))
            out.append(im2col_case(ti, to, "nchw", H, W, 3))
        for cin in (1, 3, 12):
            out.append(im2col_case(ti, to, "nhwc", 5, 7, cin))
        for how in ("kp", "nchw", "offset", "batch"):
            out.append(im2col_case(ti, to, how, 5, 7, 8))
        for cin, how in ((16, "nhwc"), (3, "nchw")):
            out.append(im2col_case(ti, to, how, 5, 7, cin, bn=True))
            out.append(im2col_case(ti, to, how, 6, 4, cin, bn=True, gelu=True))
    for dt in DTYPES:
        for i, (H, W) in enumerate(PLANES):
            out.append(col2im_vec_case(dt, H, W, 16 if i % 2 else 8, acc=bool(i % 2)))
            out.append(conv_s1_case(dt, H, W, 8 if i % 2 else 16, acc=not i % 2))
        out.append(col2im_vec_case(dt, 5, 7, 8, True, "gelu"))
        out.append(col2im_vec_case(dt, 6, 4, 16, False, "bn-gelu"))
        out += [weight_pack_case(dt, 3), weight_pack_case(dt, 8)]
    for ti, to in COL2IM_GEN_PAIRS:
        for i, (H, W) in enumerate(PLANES):
            out.append(col2im_gen_case(ti, to, H, W, 3 if i % 2 else 1))
    out += [weight_unpack_case(3, False), weight_unpack_case(8, True)]
    return out


# ================================================================================ A. ConvFFN
FFN_FWD_TILE = {32: (8, 16), 64: (8, 8), 128: (4, 8), 256: (4, 4)}
FFN_BWD_TILE = {32: (8, 8), 64: (8, 8), 128: (8, 8), 256: (4, 8)}
FFN_FLOOR = {BF16: 4e-3, F16: 1e-3}  # test_convffn_gpu.py's floor of the chain rule


def ffn_fwd_name(dt, C, save_gelu):
    """ffn_fwd_launch: C = 32 with the GELU outputs takes the 8 x 8 tile, everything else its FfnCfg tile."""
    th, tw = (8, 8) if (C == 32 and save_gelu) else FFN_FWD_TILE[C]
    return f"ffn_fwd_kernel<{TN[dt]}, {C}, 32, {th}, {tw}, {TF[save_gelu]}>"


def ffn_dh_plan(C, R, B, H, W):
    """ffn_dh_plan: (tiles, tiles per strip, strips)."""
    th, tw = FFN_BWD_TILE[C]
    ntiles = B * -(-H // th) * -(-W // tw)
    nch = R // 32
    ns = -(-1024 // nch)
    ns = max(8, min(-(-ns // 8) * 8, -(-ntiles // 8) * 8))
    tps = -(-ntiles // ns)
    return ntiles, tps, -(-ntiles // tps)


def gelu_round_err(hp, Shp, g, dt):
    """Bound on |g_kernel - GELU(hpre)| for a GELU output that a kernel computes in fp32 from exact 16-bit h
    and rounds to 16 bits without storing it. hpre is 10 fused multiply-adds (9 taps with the identity folded
    into the centre one, the bias): |hp_k - hp| <= 2 * 11 * 2^-24 Shp, Shp the same sum on absolute values;
    |GELU'| <= 1.13 carries that to the output. The evaluation x Phi(x): Phi from Abramowitz & Stegun 7.1.26
    (|erf error| <= 1.5e-7, so 0.75e-7 on Phi) through one reciprocal, one exponential and a few fp32
    operations (8 * 2^-24 relative). The rounding to the 16-bit type: half an ulp, HALF_ULP |g| (+ 2^-25,
    half the smallest fp16 subnormal)."""
    e_hp = 2 * 11 * 2.0 ** -24 * Shp
    e_eval = hp.abs() * 0.75e-7 + 8 * 2.0 ** -24 * g.abs()
    return 1.13 * e_hp + e_eval + HALF_ULP[dt] * (g.abs() + 1.13 * e_hp + e_eval) + (2.0 ** -25 if dt == F16 else 0.0)


def _hpre64(h4, wpos, bpos):
    """DW3x3(h) + bpos + h on [B, H, W, R] fp64, and the same on absolute values."""
    w = wpos.clone()
    w[:, 1, 1] += 1.0
    hp = t1._dw_apply(h4, w, 3) + bpos
    S = t1._dw_apply(h4.abs(), w.abs(), 3) + bpos.abs()
    return hp, S


def convffn_case(dt, C, R, B, H, W, save_gelu, drop):
    """dfm_convffn_fwd stage by stage from its stored tensors, then dfm_convffn_bwd: dW2 / db2 / dls with Lin from
    stored operands, the outputs that pass through the whole chain by test_convffn_gpu.py's rule."""
    t = TN[dt]
    fwd = ffn_fwd_name(dt, C, save_gelu)
    th, tw = FFN_BWD_TILE[C]
    geom = ln_geom(dt, C)
    ln = f"ln_bwd_vec_kernel<{t}, {geom[1]}, {geom[2]}>" if geom[0] == "vec" else f"ln_bwd_kernel<{t}, {geom[1]}>"
    # R is a multiple of 128: the depthwise backward scatters by rows
    bwd = frozenset([f"ffn_dhpre_kernel<{t}, {C}, 32, {th}, {tw}>", f"residual_bwd_kernel<{t}>",
                     f"dw3_rows_bwd_kernel<{t}>", ln, "partial_sum_group_kernel"])
    cid = f"convffn-{SHORT[dt]}-c{C}-r{R}-{B}x{H}x{W}-g{int(save_gelu)}-{'drop' if drop else 'keep'}"

    def run():
        import test_convffn_gpu as tcf
        g, k = gen(cid), K()
        P = B * H * W
        rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc  # noqa: E731
        p = dict(ln_w=1.0 + 0.2 * rn(C), ln_b=0.1 * rn(C), w1=rn(R, C, sc=C ** -0.5).to(dt).float(), b1=0.1 * rn(R),
                 wpos=rn(R, 1, 3, 3, sc=1 / 3), bpos=0.1 * rn(R), w2=rn(C, R, sc=R ** -0.5).to(dt).float(),
                 b2=0.1 * rn(C),
                 ls=0.5 + 0.5 * torch.rand(C, generator=g))
        x0, dout0 = rn(P, C).to(dt), rn(P, C, sc=0.5).to(dt)
        rs0 = torch.tensor([0.0, 1.25] * B)[:B] if drop else None
        dv = {kk: v.to(DEV) for kk, v in p.items()}
        w1h, w2h = dv["w1"].to(dt), dv["w2"].to(dt)
        wp9 = dv["wpos"].reshape(R, 9).contiguous()
        x, dout = x0.to(DEV), dout0.to(DEV)
        rsd = rs0.to(DEV) if drop else None
        with kv.Trace() as ta:
            res = k.convffn_fwd(x, (B, H, W), dv["ln_w"], dv["ln_b"], w1h, dv["b1"], wp9, dv["bpos"], w2h, dv["b2"],
                                dv["ls"], rowscale=rsd, save_gelu=save_gelu)
        out, f, h, xn, mean, rstd = res[:6]
        with kv.Trace() as tb:
            grads = k.convffn_bwd(dout, x, h, xn, f, mean, rstd, (B, H, W), dv["ln_w"], dv["ln_b"], w1h, wp9,
                                  dv["bpos"], w2h, dv["ls"], rowscale=rsd)
        dx, dln_w, dln_b, dw1, db1, dwpos, dbpos, dw2, db2, dls = grads
        # the 16-bit df the backward worked from: the same kernel on the same operands (deterministic)
        df, _ = k.residual_bwd(dout, f, dv["ls"], rsd, H * W)
        torch.cuda.synchronize()
        u, tol = U_OUT[dt], TOL[dt]
        P64 = {kk: d64(v) for kk, v in p.items()}
        X = d64(x0)
        mu = X.mean(1)
        var = X.var(1, unbiased=False)
        xn_ref = (X - mu[:, None]) / (var[:, None] + 1e-6).sqrt() * P64["ln_w"] + P64["ln_b"]
        checks = [Rel("mean", mean, mu, TOL[F32]), Rel("rstd", rstd, 1.0 / (var + 1e-6).sqrt(), TOL[F32]),
                  Rel("xn", xn, xn_ref, tol)]
        XN, Hk, Fk = d64(xn.cpu()), d64(h.cpu()), d64(f.cpu())  # each stage from the stored copy of its input
        checks.append(Lin("h", h, XN @ P64["w1"].t() + P64["b1"], XN.abs() @ P64["w1"].abs().t() + P64["b1"].abs(),
                          C + 1, u))
        hp, Shp = _hpre64(Hk.view(B, H, W, R), P64["wpos"].view(R, 3, 3), P64["bpos"])
        hp, Shp = hp.reshape(P, R), Shp.reshape(P, R)
        G = gelu64(hp)
        Eg = gelu_round_err(hp, Shp, G, dt)
        W2 = P64["w2"]
        # f: R products, the four waves' partial sums and the bias (n = R + 5)
        if save_gelu:
            Gk = d64(res[6].cpu())
            checks += [Rel("gelu_out", res[6], G, tol), Rel("gelu_grad", res[7], gelu_grad64(hp), tol),
                       Lin("f", f, Gk @ W2.t() + P64["b2"], Gk.abs() @ W2.abs().t() + P64["b2"].abs(), R + 5, u)]
        else:  # g is not stored: its rounding rides through |W2| (gelu_round_err)
            checks.append(Lin("f", f, G @ W2.t() + P64["b2"], G.abs() @ W2.abs().t() + P64["b2"].abs(), R + 5, u,
                              Eg @ W2.abs().t()))
        rr = d64(rs0).repeat_interleave(H * W)[:, None] if drop else torch.ones(P, 1, dtype=torch.float64)
        sc = rr * P64["ls"]
        # The epilogue adds the fp32 f it holds in registers; the stored f is that value rounded to 16 bits. So
        # out differs from x + scale * (stored f) by up to |scale| times half an ulp of f, HALF_ULP |f| (and half
        # the smallest fp16 subnormal).
        f_round = sc.abs() * (HALF_ULP[dt] * Fk.abs() + (2.0 ** -25 if dt == F16 else 0.0))
        checks.append(Lin("out", out, X + sc * Fk, X.abs() + (sc * Fk).abs(), 3, u, f_round))
        # ---- backward, from stored operands
        DO, DF = d64(dout0), d64(df.cpu())
        _, tps, nstrip = ffn_dh_plan(C, R, B, H, W)
        tl = DO * Fk * rr
        checks += [Lin("dls", dls, tl.sum(0), tl.abs().sum(0), 3 * P, U_OUT[F32]),
                   Lin("db2", db2, DF.sum(0), DF.abs().sum(0), P + nstrip, U_OUT[F32]),
                   # dW2 = df^T g with g recomputed and rounded inside the dhpre pass: gelu_round_err through |df|
                   Lin("dw2", dw2, DF.t() @ G, DF.abs().t() @ G.abs(), P + nstrip, U_OUT[F32], DF.abs().t() @ Eg)]
        # ---- backward, whole chain: against fp64 of the whole operation, the margin sized by the unfused chain
        out64, x64, d64p = tcf.ref64(p, x0, (B, H, W), rs0)
        out64.backward(DO)
        _, udx, ug = tcf.run_fn(dv, x, dout, (B, H, W), rsd, False)
        torch.cuda.synchronize()
        floor = FFN_FLOOR[dt]
        for name, got, unf, ref in (("dx", dx, udx, x64.grad), ("dln_w", dln_w, ug["ln_w"], d64p["ln_w"].grad),
                                    ("dln_b", dln_b, ug["ln_b"], d64p["ln_b"].grad),
                                    ("dw1", dw1, ug["w1"], d64p["w1"].grad),
                                    ("db1", db1, ug["b1"], d64p["b1"].grad),
                                    ("dwpos", dwpos.view(R, 1, 3, 3), ug["wpos"], d64p["wpos"].grad),
                                    ("dbpos", dbpos, ug["bpos"], d64p["bpos"].grad)):
            eu = ((unf.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()
            checks.append(Rel(name, got, ref, max(1.5 * eu, floor)))
        return (ta.names, tb.names), checks

    t1.SPLIT[cid] = (frozenset([fwd]), bwd)
    COMPOSITE[cid] = True
    return Case(cid, "convffn", frozenset([fwd]) | bwd, run)


def convffn_cases():
    out = []
    i = 0
    for dt in HALF:
        for C in (32, 64, 128, 256):
            for sg in (False, True):
                # 9 x 17: one past every tile height 4 / 8 and width 4 / 8 / 16
                out.append(convffn_case(dt, C, 256 if i % 2 else 128, 2, 9, 17, sg, drop=bool(i % 3 == 0)))
                # 1 x 1 and a plane shorter than the tile on one axis, two images (halos across the image boundary)
                small = (1, 1) if sg else (5, 3)
                out.append(convffn_case(dt, C, 128 if i % 2 else 256, 2, *small, sg, drop=bool(i % 3 == 1)))
                i += 1
        # 45 tiles over 32 wanted strips: 2 tiles per strip, 23 strips, the last with one tile
        assert ffn_dh_plan(64, 1024, 5, 17, 17) == (45, 2, 23)
        out.append(convffn_case(dt, 64, 1024, 5, 17, 17, False, drop=True))
        # the other end: one tile, 7 of the 8 launched strips empty
        assert ffn_dh_plan(128, 128, 1, 5, 3) == (1, 1, 1)
        out.append(convffn_case(dt, 128, 128, 1, 5, 3, True, drop=False))
    return out


CASES = elementwise_cases() + group_cases() + conv_cases() + convffn_cases()
assert len({c.id for c in CASES}) == len(CASES)
assert not {c.id for c in CASES} & {c.id for c in t1.CASES}


def declared():
    """Every kernel name some case of this module pins."""
    return frozenset().union(*[c.names for c in CASES])


def _family(launched, names):
    """The launched kernels that are instantiations of the templates `names` are instantiations of."""
    templates = {template_name(n) for n in names}
    return {n for n in launched if template_name(n) in templates}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_variant_tier2(case):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    library, _ = kv.library_variants()
    launched, checks = case.run()
    torch.cuda.synchronize()
    composite = case.id in COMPOSITE
    if isinstance(launched, tuple):  # a forward and a backward call: each launches its own part
        for got, want in zip(launched, t1.SPLIT[case.id]):
            got = _family(got, want) if composite else got
            assert got == want, (case.id, sorted(got), sorted(want))
        launched = launched[0] | launched[1]
    assert launched <= set(library), sorted(launched - set(library))
    pinned = _family(launched, case.names) if composite else launched
    assert pinned == case.names, (case.id, sorted(pinned), sorted(case.names))
    worst = {c.what: t1._check(case.id, c) for c in checks}
    print(f"VARIANT {case.family} {case.id} worst err/bound " +
          " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (case.id, bad)
