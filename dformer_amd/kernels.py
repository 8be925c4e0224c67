"""Thin tensor-level wrappers over the C ABI (allocation of outputs / workspaces + launch).

All tensors are CUDA (HIP) tensors; 2-D operands are [rows, cols] views whose last stride is 1
(the row stride is passed through as `ld`, so column slices of wider buffers work in place).
Activations are float32 or bfloat16; statistics / params / param-grads are float32.
"""
import ctypes
from typing import NamedTuple

import torch

from . import _lib, streams
from ._lib import check, dtype_code, lib, ptr, stream

_ws_cache = {}

# When set to a list, every GEMM launch appends its descriptor fields (tools/gemm_sweep.py)
GEMM_TRACE = None


# ---------------------------------------------------------------- accounting (bench.py)
# When ACCOUNT is a list, every wrapper appends (kernel funcs launched, algorithmic FLOPs, algorithmic
# HBM bytes, MFMA peak class) after its C call: the FLOPs/bytes an ideal kernel for that op must do
# (inputs read once, outputs written once; workspaces and split-K partials are not algorithmic).
# The library's launch tracer says which kernels the call enqueued; the first one is charged.
ACCOUNT = None
TAG = ""  # component label of the launches that follow (set by the modules; census breakdown)
_FUNCS = (ctypes.c_void_p * 64)()


def trace(flags, probe=None):
    """Launch tracer of the library: flags 0 off, 1 record launched kernels, 2 time (HIP events) the
    kernel(s) named `probe` (demangled, as rocprofv3 prints it; a name or a list of names; None = every
    kernel), 3 both."""
    if isinstance(probe, (list, tuple)):
        probe = "\n".join(probe)
    check(lib.dfm_trace_set(flags, probe.encode() if probe else None), "dfm_trace_set")


def trace_read():
    """[(kernel name, ms)] of the timed launches since the last read (synchronises on the last one)."""
    cap = 1 << 16
    funcs = (ctypes.c_void_p * cap)()
    ms = (ctypes.c_float * cap)()
    n = lib.dfm_trace_read(funcs, ms, cap)
    return [(kernel_name(funcs[i]), float(ms[i])) for i in range(min(n, cap))]


_NAMES = {}


def kernel_name(func):
    nm = _NAMES.get(func)
    if nm is None:
        nm = _NAMES[func] = lib.dfm_kernel_name(func).decode()
    return nm


def _acct(flops, nbytes, peak="bf16"):
    n = lib.dfm_trace_take(_FUNCS, 64)
    ACCOUNT.append((tuple(_FUNCS[i] for i in range(min(n, 64))), float(flops), float(nbytes), peak, TAG))


def _es(t):
    return t.element_size()


def _pref(ps):
    return None if ps is None else ctypes.byref(ps)


def _ws(nbytes, dev):
    """Scratch buffer per (device, stream) that only grows (the library never allocates); one per
    stream so kernels running concurrently on a side stream never share a workspace. A buffer that
    is outgrown is retired, not freed: a HIP graph captured earlier keeps using its pointer."""
    if nbytes == 0:
        return None
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:  # a captured graph may still hold the old pointer: never free it
            _ws_retired.append(buf)
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _ws_cache[key] = buf
    return buf


_ws_retired = []


def ld(t):
    assert t.dim() >= 2 and t.stride(-1) == 1, "inner dimension must be contiguous"
    return t.stride(-2)


def rows_of(t):
    return t.numel() // t.shape[-1] if t.is_contiguous() else t.shape[0]


# ------------------------------------------------------------------------------------------ GEMM
# ------------------------------------------------------------------ grouped weight gradients
# Inside `with wgrad_group():` the weight-gradient GEMMs (linear_wgrad) are not launched one by one:
# they are queued and issued at the end of the block as grouped launches (dfm_gemm_group, up to 8
# problems each + one split-K combine), so the independent dW GEMMs of a Block's backward share the
# chip instead of each splitting K over all of it. Their outputs must not be read before the block
# ends (they only feed the optimizer).
# The second stages of the parameter-gradient reductions issued inside (LayerNorm dgamma / dbeta,
# layer-scale dscale, depthwise dw / db: fixed-order sums over per-block partials) are deferred the
# same way and issued as ONE dfm_partial_sum_group launch per block instead of one small launch each;
# every deferred reduction keeps its own partials buffer until then.
_WG_PENDING = None
_RED_PENDING = None


WG_STREAM_MIN_FLOPS = 4e9


class wgrad_group:
    """Queue the weight-gradient GEMMs and reduction second stages issued inside; at exit issue
    them (flush_wgrad, flush_reductions) on the current stream, or on `stream` (after it waits for
    the current one), so that the current stream's later work does not wait for them."""

    def __init__(self, stream=None):
        self.stream = stream

    def __enter__(self):
        global _WG_PENDING, _RED_PENDING
        self.prev = (_WG_PENDING, _RED_PENDING)
        _WG_PENDING, _RED_PENDING = [], []
        return self

    def __exit__(self, exc_type, exc, tb):
        global _WG_PENDING, _RED_PENDING
        pending, reds = _WG_PENDING, _RED_PENDING
        _WG_PENDING, _RED_PENDING = self.prev
        if exc_type is None and (pending or reds):
            # a group worth less than WG_STREAM_MIN_FLOPS stays on the current stream: its launches take
            # about as long as the two cross-stream edges cost. Every group on the stream: DFormer-Tiny bs 8
            # (~2.5 GFLOP groups) 628.1 / 625.0 vs 639.9 / 639.0 images/s with none; from 8 GFLOP up: Tiny
            # 642.4 / 639.8 vs 639.5 / 638.7, DFormer-B flat (its ~5 GFLOP depth-branch ConvFFN groups stay);
            # from 4 GFLOP up: Tiny 651.2 / 649.5 vs 640.4 / 639.2, DFormer-B 496.9 / 504.7 vs 496.4 / 495.0
            if self.stream is None or sum(it.flops for it in pending) < WG_STREAM_MIN_FLOPS:
                _flush(pending, reds)
            else:  # operands written on the current stream, read on this one
                with streams.fork(self.stream, reads=[t for it in pending for t in (it.a, it.b)]):
                    _flush(pending, reds)
        return False


def _red_ws(nbytes, dev):
    """(workspace, DfmPartialSum or None): inside a wgrad_group a reduction gets a partials buffer of
    its own and a descriptor its entry point fills instead of launching the second stage."""
    if _RED_PENDING is None or nbytes == 0:
        return _ws(nbytes, dev), None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ps = _lib.PartialSum()
    _RED_PENDING.append((ps, buf))
    return buf, ps


def flush_reductions(reds):
    """Issue deferred reduction second stages as one dfm_partial_sum_group launch (16 per launch)."""
    n = len(reds)
    arr = (_lib.PartialSum * n)(*[r[0] for r in reds])
    cur = torch.cuda.current_stream()
    for _, buf in reds:  # partials written on a side stream are read here: no reuse before that
        buf.record_stream(cur)
    check(lib.dfm_partial_sum_group(n, ctypes.cast(arr, ctypes.c_void_p), stream()), "dfm_partial_sum_group")
    if ACCOUNT is not None:  # second stages: no algorithmic bytes (the partials are not algorithmic)
        _acct(0, 0)


class _GemmItem(NamedTuple):
    """One GEMM ready to launch: from gemm_many's `collect=` or a wgrad_group's queue. `colsum` and `bias`
    are only held so the tensors `desc` points at stay referenced until the launch."""
    desc: _lib.GemmDesc
    dtype: int
    a: torch.Tensor
    b: torch.Tensor
    out: torch.Tensor
    flops: float
    nbytes: int
    peak: str
    colsum: object = None
    bias: object = None


def _launch_gemm(it):
    ws = _ws(lib.dfm_gemm_workspace_size(it.desc), it.a.device)
    it.desc.workspace_bytes = ws.numel() if ws is not None else 0
    check(lib.dfm_gemm(it.dtype, it.desc, ptr(it.a), ptr(it.b), ptr(it.out), ptr(ws), stream()), "dfm_gemm")
    if ACCOUNT is not None:
        _acct(it.flops, it.nbytes, it.peak)


def _launch_gemm_group(chunk):
    """Up to 8 GEMMs of one dtype as one dfm_gemm_group launch."""
    n = len(chunk)
    descs = (_lib.GemmDesc * n)(*[it.desc for it in chunk])
    pa = (ctypes.c_void_p * n)(*[it.a.data_ptr() for it in chunk])
    pb = (ctypes.c_void_p * n)(*[it.b.data_ptr() for it in chunk])
    pc = (ctypes.c_void_p * n)(*[it.out.data_ptr() for it in chunk])
    ws = _ws(lib.dfm_gemm_group_workspace_size(n, descs), chunk[0].a.device)
    descs[0].workspace_bytes = ws.numel() if ws is not None else 0
    check(lib.dfm_gemm_group(chunk[0].dtype, n, descs, ctypes.cast(pa, ctypes.c_void_p), ctypes.cast(pb, ctypes.c_void_p),
                             ctypes.cast(pc, ctypes.c_void_p), ptr(ws), stream()), "dfm_gemm_group")
    if ACCOUNT is not None:
        _acct(sum(it.flops for it in chunk), sum(it.nbytes for it in chunk), chunk[0].peak)


def _launch_gemm_chunks(items):
    for i in range(0, len(items), 8):
        _launch_gemm_group(items[i:i + 8])


def flush_wgrad(pending):
    """Issue queued GEMMs as grouped launches: problems of one dtype / operand layout, 8 per launch."""
    classes = {}
    for it in pending:
        classes.setdefault((it.dtype, it.desc.a_kcontig, it.desc.b_kcontig), []).append(it)
    for items in classes.values():
        _launch_gemm_chunks(items)


def _flush(pending, reds):
    if pending:
        flush_wgrad(pending)
    if reds:
        flush_reductions(reds)


def gemm(a, b, *, M, N, K, a_kcontig, b_kcontig, lda, ldb, out, ldc, batch=1, stride_a=0, stride_b=0,
         stride_c=0, alpha=1.0, beta=0.0, bias=None, act=0, preact=None, ldpre=0, mul=None, ldmul=0, res=None,
         ldres=0, colscale=None, rowscale=None, rows_per_scale=1, split_k=0, act_col0=0, colsum=None,
         colsum_accumulate=False, mul_gelu_grad=False, mul2=None, out2=None, defer=False, collect=None):
    """One dfm_gemm launch. defer=True (weight gradients) inside `with wgrad_group():` queues it for
    the block's grouped launch instead; `collect` (a list, from gemm_many) receives it unlaunched."""
    dt = dtype_code(a)
    assert b.dtype == a.dtype, (a.dtype, b.dtype)
    c_f32 = int(out.dtype == torch.float32 and a.dtype != torch.float32)
    if out.dtype != torch.float32:
        assert out.dtype == a.dtype
    d = _lib.GemmDesc(M, N, K, batch, int(a_kcontig), int(b_kcontig), lda, ldb, ldc, stride_a, stride_b, stride_c,
                      alpha, beta, c_f32, ptr(bias), act, ptr(preact), ldpre, ptr(mul), ldmul, ptr(res), ldres,
                      ptr(colscale), ptr(rowscale), rows_per_scale, split_k, act_col0, ptr(colsum),
                      int(colsum_accumulate), int(mul_gelu_grad), 0, ptr(mul2), ld(mul2) if mul2 is not None else 0,
                      ptr(out2), ld(out2) if out2 is not None else 0)
    if GEMM_TRACE is not None:
        GEMM_TRACE.append({f: getattr(d, f) for f, _ in d._fields_ if not f in ("alpha", "beta")} |
                          {"dtype": dt, "beta": d.beta, "out_f32": out.dtype == torch.float32})
    es, nb = _es(a), max(batch, 1)
    byt = es * (M * K * nb + N * K * (nb if stride_b else 1))
    byt += M * N * nb * (out.element_size() * (2 if beta != 0.0 else 1))
    byt += es * M * N * nb * ((preact is not None) + (mul is not None) + (res is not None) + 2 * (out2 is not None))
    byt += 4 * N * (bias is not None) + 4 * M * (colsum is not None)
    peak = "bf16" if a.dtype != torch.float32 else "f32"
    it = _GemmItem(d, dt, a, b, out, 2.0 * M * N * K * nb, byt, peak, colsum, bias)
    if collect is not None:
        collect.append(it)
    elif defer and _WG_PENDING is not None:
        _WG_PENDING.append(it)  # for the block's grouped launch; the tensors stay referenced until it is issued
    else:
        _launch_gemm(it)
    return out


def gemm_many(calls):
    """Run independent GEMMs (thunks that call linear / linear_dgrad with collect=lst) as ONE grouped
    launch (dfm_gemm_group: k-contiguous A problems go to the LDS-DMA ring kernel's grouped variant);
    a single call launches alone. The calls must not read each other's outputs."""
    items = []
    for c in calls:
        c(items)
    if len(items) == 1:
        _launch_gemm(items[0])
    else:
        _launch_gemm_chunks(items)


def linear(x, w, bias=None, *, act=0, preact=None, mul=None, res=None, colscale=None, rowscale=None,
           rows_per_scale=1, out=None, beta=0.0, act_col0=0, collect=None):
    """y[M,N] = epi(x[M,K] @ w[N,K]^T)  (nn.Linear forward)."""
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=x.dtype)
    return gemm(x, w, M=M, N=N, K=K, a_kcontig=True, b_kcontig=True, lda=ld(x), ldb=ld(w), out=out, ldc=ld(out),
                beta=beta, bias=bias, act=act, preact=preact, ldpre=ld(preact) if preact is not None else 0,
                mul=mul, ldmul=ld(mul) if mul is not None else 0, res=res, ldres=ld(res) if res is not None else 0,
                colscale=colscale, rowscale=rowscale, rows_per_scale=rows_per_scale, act_col0=act_col0,
                collect=collect)


def linear_dgrad(dy, w, out=None, accumulate=False, mul=None, gelu_grad_of=None, mul2=None, out2=None,
                 collect=None):
    """dx[M,K] (+)= dy[M,N] @ w[N,K]   (times `mul` elementwise, or times gelu'(gelu_grad_of)); with
    mul2 / out2 also out2 = (dy @ w) * mul2 from the same accumulator (an elementwise product's two
    input gradients in one pass: out = g * y, out2 = g * x for the product x * y)."""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, device=dy.device, dtype=dy.dtype)
    if gelu_grad_of is not None:
        mul = gelu_grad_of
    return gemm(dy, w, M=M, N=K, K=N, a_kcontig=True, b_kcontig=False, lda=ld(dy), ldb=ld(w), out=out, ldc=ld(out),
                beta=1.0 if accumulate else 0.0, mul=mul, ldmul=ld(mul) if mul is not None else 0,
                mul_gelu_grad=gelu_grad_of is not None, mul2=mul2, out2=out2, collect=collect)


def linear_wgrad(dy, x, out=None, accumulate=False, bias_grad=False, bias_out=None):
    """dW[N,K] (+)= dy[M,N]^T @ x[M,K]  (float32 output, split-K over M).
    bias_grad=True also returns db[N] = sum_M dy (fused: virtual all-ones column of x), written
    into `bias_out` when given (e.g. a slot of the optimizer's flat gradient buffer)."""
    M, N = dy.shape
    K = x.shape[1]
    if out is None:
        out = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = None
    if bias_grad:
        db = bias_out if bias_out is not None else torch.empty(N, device=dy.device, dtype=torch.float32)
    gemm(dy, x, M=N, N=K, K=M, a_kcontig=False, b_kcontig=False, lda=ld(dy), ldb=ld(x), out=out,
         ldc=ld(out), beta=1.0 if accumulate else 0.0, colsum=db, colsum_accumulate=accumulate, defer=True)
    return (out, db) if bias_grad else out


def bmm(a, b, *, a_t=False, b_t=False, out=None, alpha=1.0, beta=0.0):
    """Batched out[b] (= or +=) op(a[b]) @ op(b[b]) for contiguous 3-D tensors (op = transpose if *_t)."""
    B = a.shape[0]
    M = a.shape[2] if a_t else a.shape[1]
    K = a.shape[1] if a_t else a.shape[2]
    N = b.shape[1] if b_t else b.shape[2]
    assert (b.shape[2] if b_t else b.shape[1]) == K
    if out is None:
        out = torch.empty(B, M, N, device=a.device, dtype=a.dtype)
    # A(m,k): a[m][k] (k-contig, lda=K) or a[k][m] (a_t: row-contig, lda=M)
    # B(k,n): b[k][n] (row-contig, ldb=N) or b[n][k] (b_t: k-contig, ldb=K)
    return gemm(a, b, M=M, N=N, K=K, a_kcontig=not a_t, b_kcontig=b_t, lda=a.shape[2], ldb=b.shape[2], out=out,
                ldc=N, batch=B, stride_a=a.shape[1] * a.shape[2], stride_b=b.shape[1] * b.shape[2],
                stride_c=M * N, alpha=alpha, beta=beta)


# ------------------------------------------------------------------------------------ LayerNorm
def layernorm(x, gamma, beta, eps=1e-6, out=None):
    rows, C = x.shape
    if out is None:
        out = torch.empty(rows, C, device=x.device, dtype=x.dtype)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib.dfm_layernorm_fwd(dtype_code(x), rows, C, ptr(x), ld(x), ptr(gamma), ptr(beta), eps, ptr(out),
                                ld(out), ptr(mean), ptr(rstd), stream()), "dfm_layernorm_fwd")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * 2 + 8 * rows)
    return out, mean, rstd


def layernorm_bwd(x, dy, gamma, mean, rstd, dx=None, accumulate=False, dres=None):
    """dx = LN'(dy) [+ dres] [+ dx when accumulate]; returns (dx, dgamma, dbeta)."""
    rows, C = x.shape
    if dx is None:
        dx = torch.empty(rows, C, device=x.device, dtype=x.dtype)
        accumulate = False
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws, ps = _red_ws(lib.dfm_layernorm_bwd_workspace(rows, C), x.device)
    check(lib.dfm_layernorm_bwd(dtype_code(x), rows, C, ptr(x), ld(x), ptr(dy), ld(dy), ptr(gamma), ptr(mean),
                                ptr(rstd), ptr(dres), ld(dres) if dres is not None else 0, ptr(dx), ld(dx),
                                int(accumulate), ptr(dg), ptr(db), ptr(ws), _pref(ps), stream()), "dfm_layernorm_bwd")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * (3 + (dres is not None) + bool(accumulate)) + 8 * rows)
    return dx, dg, db


def layernorm_bwd_pool(x, dy, gamma, mean, rstd, pooled, shape, dres=None):
    """layernorm_bwd of dy + pool7_bwd(pooled) (the sum rounded to the dtype, as pool7_bwd(accumulate=True) leaves it
    in dy): bit-identical to that pair, in one launch where the vector LayerNorm kernel applies (dy is then left
    as it was; elsewhere the entry point issues the pair and dy receives the sum). Returns (dx, dgamma, dbeta)."""
    B, H, W = shape
    rows, C = x.shape
    dx = torch.empty(rows, C, device=x.device, dtype=x.dtype)
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws, ps = _red_ws(lib.dfm_layernorm_bwd_workspace(rows, C), x.device)
    check(lib.dfm_layernorm_bwd_pool(dtype_code(x), rows, C, ptr(x), ld(x), ptr(dy), ld(dy), ptr(gamma), ptr(mean),
                                     ptr(rstd), ptr(dres), ld(dres) if dres is not None else 0, ptr(dx), ld(dx), 0,
                                     ptr(dg), ptr(db), ptr(ws), _pref(ps), ptr(pooled), ld(pooled), B, H, W, stream()),
          "dfm_layernorm_bwd_pool")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * (3 + (dres is not None)) + 8 * rows + B * 49 * C * _es(x))
    return dx, dg, db


def residual_bwd2(dout1, f1, colscale1, rowscale1, rps1, df1, dout2, f2, colscale2, rowscale2, rps2, df2):
    """Two residual_bwd problems in one launch (the attention backward's proj / proj_e pair): every result
    bit-identical to two residual_bwd calls. Returns (dls1, dls2)."""
    prob = []
    for dout, f, cs, rs, rps, df in ((dout1, f1, colscale1, rowscale1, rps1, df1),
                                     (dout2, f2, colscale2, rowscale2, rps2, df2)):
        rows, C = dout.shape
        dls = torch.empty(C, device=dout.device, dtype=torch.float32)
        ws, ps = _red_ws(lib.dfm_residual_bwd_workspace(rows, C), dout.device)
        if ps is None and prob:  # outside a wgrad_group the stream's scratch serves one problem: its own buffer
            ws = torch.empty(lib.dfm_residual_bwd_workspace(rows, C), dtype=torch.uint8, device=dout.device)
        prob.append((dls, ps, [rows, C, ptr(dout), ld(dout), ptr(f), ld(f), ptr(cs), ptr(rs), rps, ptr(df), ld(df),
                               ptr(dls), ptr(ws), _pref(ps)], ws))
    check(lib.dfm_residual_bwd2(dtype_code(dout1), *prob[0][2], *prob[1][2], stream()), "dfm_residual_bwd2")
    if ACCOUNT is not None:
        _acct(0, sum(d.shape[0] * d.shape[1] * _es(d) * 3 for d in (dout1, dout2)))
    return prob[0][0], prob[1][0]


def residual_bwd(dout, f, colscale, rowscale=None, rows_per_scale=1, df=None):
    """Block residual x + rowscale*ls*f backward: returns (df = dout*ls*rowscale, dls = sum dout*f*rowscale)."""
    rows, C = dout.shape
    if df is None:
        df = torch.empty(rows, C, device=dout.device, dtype=dout.dtype)
    dls = torch.empty(C, device=dout.device, dtype=torch.float32)
    ws, ps = _red_ws(lib.dfm_residual_bwd_workspace(rows, C), dout.device)
    check(lib.dfm_residual_bwd(dtype_code(dout), rows, C, ptr(dout), ld(dout), ptr(f), ld(f), ptr(colscale),
                               ptr(rowscale), rows_per_scale, ptr(df), ld(df), ptr(dls), ptr(ws), _pref(ps), stream()),
          "dfm_residual_bwd")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(dout) * 3)
    return df, dls


# ----------------------------------------------------------------------------- fused ConvFFN (K4)
def _acct_named(parts, peak="bf16"):
    """Account one entry point that launched several kernels: parts = [(name substring, flops, bytes)];
    each launched kernel is charged the first unused part whose substring its name contains."""
    n = lib.dfm_trace_take(_FUNCS, 64)
    used = [False] * len(parts)
    for i in range(min(n, 64)):
        f = _FUNCS[i]
        nm = kernel_name(f)
        fl = by = 0.0
        for j, (sub, pf, pb) in enumerate(parts):
            if not used[j] and sub in nm:
                used[j], fl, by = True, pf, pb
                break
        ACCOUNT.append(((f,), float(fl), float(by), peak, TAG))


def _ffn_desc(shape, C, hidden, eps):
    B, H, W = shape
    return _lib.ConvFFNDesc(B, H, W, C, hidden, eps)


def convffn_supported(dtype, shape, C, hidden):
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    d = _ffn_desc(shape, C, hidden, 1e-6)
    code = _lib.BF16 if dtype == torch.bfloat16 else _lib.F16
    return bool(lib.dfm_convffn_supported(code, ctypes.byref(d)))


def convffn_fwd(x, shape, ln_w, ln_b, w1, b1, wpos, bpos, w2, b2, ls, rowscale=None, eps=1e-6, save_gelu=False):
    """Fused ConvFFN + Block residual (DFormer.py:48-67, 176-179). Returns (out, f, h, xn, mean, rstd)
    (+ (g, gp) = GELU(hpre), GELU'(hpre) with save_gelu, the op-level backward's operands):
    out = x + rowscale * ls * f, f = fc2 pre-residual output, h = fc1 output, LN output / statistics."""
    P, C = x.shape
    R = w1.shape[0]
    d = _ffn_desc(shape, C, R, eps)
    out, f = torch.empty_like(x), torch.empty_like(x)
    h = torch.empty(P, R, device=x.device, dtype=x.dtype)
    xn = torch.empty_like(x)
    mean = torch.empty(P, device=x.device, dtype=torch.float32)
    rstd = torch.empty(P, device=x.device, dtype=torch.float32)
    g = gp = None
    if save_gelu:
        g, gp = torch.empty_like(h), torch.empty_like(h)
    check(lib.dfm_convffn_fwd(dtype_code(x), ctypes.byref(d), ptr(x), ptr(ln_w), ptr(ln_b), ptr(w1), ptr(b1),
                              ptr(wpos), ptr(bpos), ptr(w2), ptr(b2), ptr(ls), ptr(rowscale), ptr(out), ptr(f),
                              ptr(h), ptr(xn), ptr(mean), ptr(rstd), ptr(g), ptr(gp), stream()), "dfm_convffn_fwd")
    if ACCOUNT is not None:
        es = _es(x)
        _acct(4.0 * P * C * R + 18.0 * P * R, es * P * (4 * C + R * (3 if save_gelu else 1)) + 8 * P + es * 2 * C * R)
    if save_gelu:
        return out, f, h, xn, mean, rstd, g, gp
    return out, f, h, xn, mean, rstd


def convffn_bwd(dout, x, h, xn, f, mean, rstd, shape, ln_w, ln_b, w1, wpos, bpos, w2, ls, rowscale=None, eps=1e-6,
                grads=None):
    """Backward of convffn_fwd. Returns (dx, dln_w, dln_b, dw1, db1, dwpos, dbpos, dw2, db2, dls); the
    parameter gradients go to the tensors of `grads` (same order, None = allocate; float32, overwritten)."""
    P, C = x.shape
    R = w1.shape[0]
    d = _ffn_desc(shape, C, R, eps)
    code = dtype_code(x)
    dev = x.device
    shapes = [(C,), (C,), (R, C), (R,), (R, 9), (R,), (C, R), (C,), (C,)]
    grads = list(grads) if grads is not None else [None] * 9
    outs = [g if g is not None else torch.empty(sh, device=dev, dtype=torch.float32) for g, sh in zip(grads, shapes)]
    dx = torch.empty_like(x)
    nbytes = lib.dfm_convffn_bwd_workspace_size(code, ctypes.byref(d))
    ws = _ws(nbytes, dev)
    check(lib.dfm_convffn_bwd(code, ctypes.byref(d), ptr(dout), ptr(x), ptr(h), ptr(xn), ptr(f), ptr(mean), ptr(rstd),
                              ptr(ln_w), ptr(ln_b), ptr(w1), ptr(wpos), ptr(bpos), ptr(w2), ptr(ls), ptr(rowscale),
                              ptr(dx), *[ptr(o) for o in outs], ptr(ws), nbytes, stream()), "dfm_convffn_bwd")
    if ACCOUNT is not None:
        es = _es(x)
        _acct_named([("residual", 0.0, 3.0 * es * P * C),
                     ("ffn_bwd", 6.0 * P * C * R + 36.0 * P * R, es * P * (2 * R + 2 * C) + 8 * P),
                     ("ffn_dhpre", 4.0 * P * C * R + 18.0 * P * R, es * P * (2 * R + C)),
                     ("dw3", 36.0 * P * R, es * P * 3 * R),
                     ("gemm", 2.0 * P * C * R, es * (P * R + P * C + R * C)),
                     ("gemm", 2.0 * P * C * R, es * (P * R + P * C + R * C)),
                     ("ln_bwd", 0.0, es * P * C * 4 + 8 * P)])
    return (dx, *outs)


# ---------------------------------------------------------------------------- depthwise conv
def dwconv(x, shape, w, bias, k, add_identity=False, out=None, gelu_out=None, out_gelu_grad=False):
    """x: [B*H*W, C] view (NHWC rows); w float32 [C,1,k,k] or [C,k,k]. gelu_out: also GELU(y);
    out_gelu_grad (with gelu_out): `out` receives GELU'(y) instead of y."""
    B, H, W = shape
    C = x.shape[1]
    if out is None:
        out = torch.empty(x.shape[0], C, device=x.device, dtype=x.dtype)
    flags = int(bool(add_identity)) | (2 if out_gelu_grad and gelu_out is not None else 0)
    check(lib.dfm_dwconv_fwd(dtype_code(x), B, H, W, C, k, ptr(x), ld(x), ptr(w), ptr(bias), flags,
                             ptr(out), ld(out), ptr(gelu_out), ld(gelu_out) if gelu_out is not None else 0,
                             stream()), "dfm_dwconv_fwd")
    if ACCOUNT is not None:
        _acct(2 * k * k * C * x.shape[0], x.shape[0] * C * _es(x) * (2 + (gelu_out is not None)))
    return out


def dwconv_bwd_data(dy, shape, w, k, add_identity=False, dx=None, accumulate=False):
    B, H, W = shape
    C = dy.shape[1]
    if dx is None:
        dx = torch.empty(dy.shape[0], C, device=dy.device, dtype=dy.dtype)
        accumulate = False
    check(lib.dfm_dwconv_bwd_data(dtype_code(dy), B, H, W, C, k, ptr(dy), ld(dy), ptr(w), int(add_identity),
                                  ptr(dx), ld(dx), int(accumulate), stream()), "dfm_dwconv_bwd_data")
    if ACCOUNT is not None:
        _acct(2 * k * k * C * dy.shape[0], dy.shape[0] * C * _es(dy) * (2 + bool(accumulate)))
    return dx


def dwconv_bwd_data_mul(dy, shape, w, k, mul, prior=None, add_identity=False, dx=None):
    """dx = round(round(conv(dy, flipped w) (+ dy) (+ prior)) * mul): dwconv_bwd_data (accumulating onto prior) and
    scale_mul(mul=...) in one launch, bit-identical to the pair (the inner rounding is the pair's store)."""
    B, H, W = shape
    C = dy.shape[1]
    if dx is None:
        dx = torch.empty(dy.shape[0], C, device=dy.device, dtype=dy.dtype)
    check(lib.dfm_dwconv_bwd_data_mul(dtype_code(dy), B, H, W, C, k, ptr(dy), ld(dy), ptr(w), int(add_identity),
                                      ptr(prior), ld(prior) if prior is not None else 0, ptr(mul), ld(mul), ptr(dx),
                                      ld(dx), stream()), "dfm_dwconv_bwd_data_mul")
    if ACCOUNT is not None:
        _acct(2 * k * k * C * dy.shape[0], dy.shape[0] * C * _es(dy) * (3 + (prior is not None)))
    return dx


def dwconv_bwd(x, dy, shape, w, k, add_identity=False, dx=None, accumulate=False, dw=None, db=None):
    """Input gradient and weight / bias gradient of a 3x3 depthwise conv in one pass (dfm_dwconv_bwd)."""
    B, H, W = shape
    C = x.shape[1]
    if dx is None:
        dx = torch.empty(dy.shape[0], C, device=dy.device, dtype=dy.dtype)
        accumulate = False
    if dw is None:
        dw = torch.empty(C, 1, k, k, device=x.device, dtype=torch.float32)
    if db is None:
        db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws, ps = _red_ws(lib.dfm_dwconv_bwd_weight_workspace(B, H, W, C, k), x.device)
    check(lib.dfm_dwconv_bwd(dtype_code(x), B, H, W, C, k, ptr(x), ld(x), ptr(dy), ld(dy), ptr(w), int(add_identity),
                             ptr(dx), ld(dx), int(accumulate), ptr(dw), ptr(db), ptr(ws), _pref(ps), stream()),
          "dfm_dwconv_bwd")
    if ACCOUNT is not None:
        _acct(4 * k * k * C * x.shape[0], x.shape[0] * C * _es(x) * (3 + bool(accumulate)))
    return dx, dw, db


def ffn_dgrad_dw3_supported(dtype, shape, C, hidden, operands=()):
    """Whether ffn_dgrad_dw3_bwd takes this dtype and shape and, when given, these operands (df, w2, gp, h, dh):
    the entry point wants rows of 16-byte vectors (contiguous inner dimension, row stride a multiple of 8
    elements, 16-byte aligned pointer). A caller that gets False takes the pair."""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    for t in operands:
        if t is not None and (t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16):
            return False
    B, H, W = shape
    code = _lib.BF16 if dtype == torch.bfloat16 else _lib.F16
    return bool(lib.dfm_ffn_dgrad_dw3_supported(code, B, H, W, C, hidden))


def ffn_dgrad_dw3_bwd(df, w2, gp, h, shape, wpos, add_identity=True, dh=None, dw=None, db=None):
    """dh, dwpos, dbpos of hpre = DW3x3(h) + bpos + h for dhpre = (df @ w2) * gp in one kernel: the pair
    linear_dgrad(df, w2, mul=gp) + dwconv_bwd(h, dhpre, ...) without dhpre in memory (dfm_ffn_dgrad_dw3_bwd).
    w2: the forward's fc2 weight [C, hidden]. An unsupported shape raises before any launch."""
    B, H, W = shape
    P, C = df.shape
    R = w2.shape[1]
    if dh is None:
        dh = torch.empty(P, R, device=df.device, dtype=df.dtype)
    if dw is None:
        dw = torch.empty(R, 1, 3, 3, device=df.device, dtype=torch.float32)
    if db is None:
        db = torch.empty(R, device=df.device, dtype=torch.float32)
    ws, ps = _red_ws(lib.dfm_ffn_dgrad_dw3_workspace(B, H, W, R), df.device)
    check(lib.dfm_ffn_dgrad_dw3_bwd(dtype_code(df), B, H, W, C, R, ptr(df), ld(df), ptr(w2), ld(w2), ptr(gp), ld(gp),
                                    ptr(h), ld(h), ptr(wpos), int(add_identity), ptr(dh), ld(dh), ptr(dw), ptr(db),
                                    ptr(ws), _pref(ps), stream()), "dfm_ffn_dgrad_dw3_bwd")
    if ACCOUNT is not None:
        _acct(2.0 * P * C * R + 36.0 * P * R, _es(df) * P * (C + 3 * R))
    return dh, dw, db


def dwconv_bwd_weight(x, dy, shape, k, dw=None, db=None):
    B, H, W = shape
    C = x.shape[1]
    if dw is None:
        dw = torch.empty(C, 1, k, k, device=x.device, dtype=torch.float32)
    if db is None:
        db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws, ps = _red_ws(lib.dfm_dwconv_bwd_weight_workspace(B, H, W, C, k), x.device)
    check(lib.dfm_dwconv_bwd_weight(dtype_code(x), B, H, W, C, k, ptr(x), ld(x), ptr(dy), ld(dy), ptr(dw), ptr(db),
                                    ptr(ws), _pref(ps), stream()), "dfm_dwconv_bwd_weight")
    if ACCOUNT is not None:
        _acct(2 * k * k * C * x.shape[0], x.shape[0] * C * _es(x) * 2)
    return dw, db


# -------------------------------------------------------------------------- reductions / misc
def colsum(x, mul=None, rowscale=None, rows_per_scale=1, out=None, accumulate=False):
    rows, C = x.shape
    if out is None:
        out = torch.empty(C, device=x.device, dtype=torch.float32)
        accumulate = False
    ws = _ws(lib.dfm_colsum_workspace(rows, C), x.device)
    check(lib.dfm_colsum(dtype_code(x), rows, C, ptr(x), ld(x), ptr(mul), ld(mul) if mul is not None else 0,
                         ptr(rowscale), rows_per_scale, ptr(out), int(accumulate), ptr(ws), stream()), "dfm_colsum")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * (1 + (mul is not None)))
    return out


def cast(x, dtype, out=None):
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    assert x.is_contiguous() and out.is_contiguous()
    check(lib.dfm_cast(dtype_code(x), dtype_code(out), x.numel(), ptr(x), ptr(out), stream()), "dfm_cast")
    if ACCOUNT is not None:
        _acct(0, x.numel() * (_es(x) + _es(out)))
    return out


def pack_slices(srcs, out):
    """out [..., n * cols] <- the n tensors [..., cols] side by side (converted to out.dtype), one launch."""
    n, cols = len(srcs), srcs[0].shape[-1]
    rows = srcs[0].numel() // cols
    assert out.is_contiguous() and out.shape[-1] == n * cols and out.numel() == rows * n * cols
    for t in srcs:
        assert t.is_contiguous() and t.shape[-1] == cols and t.numel() == rows * cols
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dts = (ctypes.c_int * n)(*[dtype_code(t) for t in srcs])
    check(lib.dfm_pack_slices(dtype_code(out), n, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(dts, ctypes.c_void_p),
                              rows, cols, ptr(out), stream()), "dfm_pack_slices")
    if ACCOUNT is not None:
        _acct(0, sum(t.numel() * _es(t) for t in srcs) + out.numel() * _es(out))
    return out


def gelu_bwd(dy, pre, out=None, accumulate=False):
    rows, C = dy.shape
    if out is None:
        out = torch.empty(rows, C, device=dy.device, dtype=dy.dtype)
        accumulate = False
    check(lib.dfm_gelu_bwd(dtype_code(dy), rows, C, ptr(dy), ld(dy), ptr(pre), ld(pre), ptr(out), ld(out),
                           int(accumulate), stream()), "dfm_gelu_bwd")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(dy) * (3 + bool(accumulate)))
    return out


def relu_bwd(dy, y, out=None):
    rows, C = dy.shape
    if out is None:
        out = torch.empty(rows, C, device=dy.device, dtype=dy.dtype)
    check(lib.dfm_relu_bwd(dtype_code(dy), rows, C, ptr(dy), ld(dy), ptr(y), ld(y), ptr(out), ld(out), stream()),
          "dfm_relu_bwd")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(dy) * 3)
    return out


def scale_mul(src, mul=None, colscale=None, rowscale=None, rows_per_scale=1, alpha=1.0, out=None, accumulate=False):
    rows, C = src.shape
    if out is None:
        out = torch.empty(rows, C, device=src.device, dtype=src.dtype)
        accumulate = False
    check(lib.dfm_scale_mul(dtype_code(src), rows, C, ptr(src), ld(src), ptr(mul), ld(mul) if mul is not None else 0,
                            ptr(colscale), ptr(rowscale), rows_per_scale, alpha, ptr(out), ld(out), int(accumulate),
                            stream()), "dfm_scale_mul")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(src) * (2 + (mul is not None) + bool(accumulate)))
    return out


def group_scale(x, scale, rows_per_group, out=None):
    """out[r, c] = x[r, c] * scale[r // rows_per_group, c] (float32 scale [groups, C]); out may be x."""
    rows, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() >= -(-rows // rows_per_group) * C
    check(lib.dfm_group_scale(dtype_code(x), rows, C, ptr(x), ld(x), ptr(scale), rows_per_group, ptr(out), ld(out),
                              stream()), "dfm_group_scale")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * 2)
    return out


def dual_mul(src, m1, m2, out1=None, out2=None):
    """(src * m1, src * m2) in one pass over src (the two gradients of an elementwise product)."""
    rows, C = src.shape
    if out1 is None:
        out1 = torch.empty(rows, C, device=src.device, dtype=src.dtype)
    if out2 is None:
        out2 = torch.empty(rows, C, device=src.device, dtype=src.dtype)
    check(lib.dfm_dual_mul(dtype_code(src), rows, C, ptr(src), ld(src), ptr(m1), ld(m1), ptr(m2), ld(m2), ptr(out1),
                           ld(out1), ptr(out2), ld(out2), stream()), "dfm_dual_mul")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(src) * 5)
    return out1, out2


# ---------------------------------------------------------------------- pool / bilinear / attn
def pool7(x, shape, out=None):
    B, H, W = shape
    C = x.shape[1]
    if out is None:
        out = torch.empty(B * 49, C, device=x.device, dtype=x.dtype)
    check(lib.dfm_adaptive_pool7_fwd(dtype_code(x), B, H, W, C, ptr(x), ld(x), ptr(out), ld(out), stream()),
          "dfm_adaptive_pool7_fwd")
    if ACCOUNT is not None:
        _acct(0, (B * H * W + B * 49) * C * _es(x))
    return out


def pool7_pair(x1, x2, shape, out1, out2):
    """pool7(x1) into out1 and pool7(x2) into out2 (two column blocks of one buffer) in one launch."""
    B, H, W = shape
    check(lib.dfm_adaptive_pool7_fwd2(dtype_code(x1), B, H, W, x1.shape[1], ptr(x1), ld(x1), ptr(out1), ld(out1),
                                      x2.shape[1], ptr(x2), ld(x2), ptr(out2), ld(out2), stream()),
          "dfm_adaptive_pool7_fwd2")
    if ACCOUNT is not None:
        _acct(0, (B * H * W + B * 49) * (x1.shape[1] + x2.shape[1]) * _es(x1))
    return out1, out2


def pool7_bwd(dy, shape, dx=None, accumulate=False):
    B, H, W = shape
    C = dy.shape[1]
    if dx is None:
        dx = torch.empty(B * H * W, C, device=dy.device, dtype=dy.dtype)
        accumulate = False
    check(lib.dfm_adaptive_pool7_bwd(dtype_code(dy), B, H, W, C, ptr(dy), ld(dy), ptr(dx), ld(dx), int(accumulate),
                                     stream()), "dfm_adaptive_pool7_bwd")
    if ACCOUNT is not None:
        _acct(0, (B * H * W * (1 + bool(accumulate)) + B * 49) * C * _es(dy))
    return dx


def bilinear(x, in_hw, out_hw, B, out=None, accumulate=False):
    (Hi, Wi), (Ho, Wo) = in_hw, out_hw
    C = x.shape[1]
    if out is None:
        out = torch.empty(B * Ho * Wo, C, device=x.device, dtype=x.dtype)
        accumulate = False
    check(lib.dfm_bilinear_fwd(dtype_code(x), B, Hi, Wi, Ho, Wo, C, ptr(x), ld(x), ptr(out), ld(out),
                               int(accumulate), stream()), "dfm_bilinear_fwd")
    if ACCOUNT is not None:
        _acct(0, (B * Hi * Wi + B * Ho * Wo * (1 + bool(accumulate))) * C * _es(x))
    return out


def bilinear_bwd(dy, in_hw, out_hw, B, dx=None, accumulate=False):
    (Hi, Wi), (Ho, Wo) = in_hw, out_hw
    C = dy.shape[1]
    if dx is None:
        dx = torch.empty(B * Hi * Wi, C, device=dy.device, dtype=dy.dtype)
        accumulate = False
    check(lib.dfm_bilinear_bwd(dtype_code(dy), B, Hi, Wi, Ho, Wo, C, ptr(dy), ld(dy), ptr(dx), ld(dx),
                               int(accumulate), stream()), "dfm_bilinear_bwd")
    if ACCOUNT is not None:
        _acct(0, (B * Hi * Wi * (1 + bool(accumulate)) + B * Ho * Wo) * C * _es(dy))
    return dx


def pooled_attn(q, k, v, B, heads, N, dh, scale, out=None):
    """q: [B*49, >=heads*dh] view, k/v: [B*N, ...] views (head h at cols h*dh)."""
    if out is None:
        out = torch.empty(B * 49, heads * dh, device=q.device, dtype=q.dtype)
    lse = torch.empty(B * heads * 49, device=q.device, dtype=torch.float32)
    ws = _ws(lib.dfm_pooled_attn_workspace(B, heads, N, dh), q.device)
    assert ld(k) == ld(v)
    check(lib.dfm_pooled_attn_fwd(dtype_code(q), B, heads, N, dh, ptr(q), ld(q), ptr(k), ptr(v), ld(k), scale,
                                  ptr(out), ld(out), ptr(lse), ptr(ws), stream()), "dfm_pooled_attn_fwd")
    if ACCOUNT is not None:
        _acct(4.0 * B * heads * 49 * N * dh, _es(q) * (2 * B * 49 * heads * dh + 2 * B * N * heads * dh))
    return out, lse


def pooled_attn_bwd(q, k, v, o, dout, lse, B, heads, N, dh, scale, dq, dk, dv):
    ws = _ws(lib.dfm_pooled_attn_workspace(B, heads, N, dh), q.device)
    assert ld(dk) == ld(dv) and ld(dq) == ld(q)
    check(lib.dfm_pooled_attn_bwd(dtype_code(q), B, heads, N, dh, ptr(q), ld(q), ptr(k), ptr(v), ld(k), scale,
                                  ptr(o), ld(o), ptr(dout), ld(dout), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ld(dk),
                                  ptr(ws), stream()), "dfm_pooled_attn_bwd")
    if ACCOUNT is not None:
        hd = heads * dh
        _acct(10.0 * B * heads * 49 * N * dh, _es(q) * (4 * B * 49 * hd + 4 * B * N * hd))


# ---------------------------------------------------------------------------------- BatchNorm
def bn_stats(x):
    """float32 [3, C]: (sum (x-K), sum (x-K)^2, K) with the per-column shift K = x[0]."""
    rows, C = x.shape
    st = torch.empty(3, C, device=x.device, dtype=torch.float32)
    ws = _ws(lib.dfm_bn_workspace(rows, C), x.device)
    check(lib.dfm_bn_stats(dtype_code(x), rows, C, ptr(x), ld(x), ptr(st), ptr(ws), stream()), "dfm_bn_stats")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x))
    return st


def bn_finalize(stats, count, eps, momentum, running_mean=None, running_var=None):
    C = stats.shape[1]
    mean = torch.empty(C, device=stats.device, dtype=torch.float32)
    rstd = torch.empty(C, device=stats.device, dtype=torch.float32)
    check(lib.dfm_bn_finalize(C, ptr(stats), float(count), eps, momentum, ptr(mean), ptr(rstd), ptr(running_mean),
                              ptr(running_var), stream()), "dfm_bn_finalize")
    if ACCOUNT is not None:
        _acct(0, C * 4 * (3 + 4 * (running_mean is not None)))
    return mean, rstd


def bn_merge(parts, counts):
    """SyncBN: all-gathered per-rank bn_stats triples [S, 3, C] + per-rank rows [S] (float32) -> the
    union's triple [3, C], shifted by rank 0's K (fixed order; identity for S = 1)."""
    S, three, C = parts.shape
    if three != 3 or counts.shape != (S,) or parts.dtype != torch.float32 or counts.dtype != torch.float32:
        raise ValueError(f"bn_merge: parts {tuple(parts.shape)} {parts.dtype}, counts {tuple(counts.shape)}")
    parts, counts = parts.contiguous(), counts.contiguous()
    st = torch.empty(3, C, device=parts.device, dtype=torch.float32)
    check(lib.dfm_bn_merge(S, C, ptr(parts), ptr(counts), ptr(st), stream()), "dfm_bn_merge")
    return st


def bn_apply(x, mean, rstd, gamma, beta, res=None, act=0, out=None):
    rows, C = x.shape
    if out is None:
        out = torch.empty(rows, C, device=x.device, dtype=x.dtype)
    check(lib.dfm_bn_apply(dtype_code(x), rows, C, ptr(x), ld(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                           ptr(res), ld(res) if res is not None else 0, act, ptr(out), ld(out), stream()),
          "dfm_bn_apply")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * (2 + (res is not None)))
    return out


def bn_bwd_stats(x, dy, mean, rstd, out=None):
    rows, C = x.shape
    st = torch.empty(2, C, device=x.device, dtype=torch.float32) if out is None else out
    ws = _ws(lib.dfm_bn_workspace(rows, C), x.device)
    check(lib.dfm_bn_bwd_stats(dtype_code(x), rows, C, ptr(x), ld(x), ptr(dy), ld(dy), ptr(mean), ptr(rstd),
                               ptr(st), ptr(ws), stream()), "dfm_bn_bwd_stats")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * 2)
    return st


def bn_bwd_apply(x, dy, mean, rstd, gamma, stats2, count, dx=None, accumulate=False):
    rows, C = x.shape
    if dx is None:
        dx = torch.empty(rows, C, device=x.device, dtype=x.dtype)
        accumulate = False
    check(lib.dfm_bn_bwd_apply(dtype_code(x), rows, C, ptr(x), ld(x), ptr(dy), ld(dy), ptr(mean), ptr(rstd),
                               ptr(gamma), ptr(stats2), float(count), ptr(dx), ld(dx), int(accumulate), stream()),
          "dfm_bn_bwd_apply")
    if ACCOUNT is not None:
        _acct(0, rows * C * _es(x) * (3 + bool(accumulate)))
    return dx


# ------------------------------------------------- dense 3x3 conv (stride 2: stems; stride 1: aux head)
def conv3s2_kp(cin):
    """Packed K (columns of the gathered operand): 9*cin rounded up to a multiple of 8."""
    return (9 * cin + 7) // 8 * 8


def conv3s2_im2col(x, dtype, bn=None, gelu=False, out=None):
    """Gather of nn.Conv2d(cin, cout, 3, 2, 1)'s operand from an NCHW-logical tensor x (any strides),
    with an optional folded BatchNorm affine bn = (mean, rstd, gamma, beta) and exact GELU.
    Returns cols [B*Ho*Wo, Kp] in `dtype` (columns (kh, kw, c))."""
    B, C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    kp = conv3s2_kp(C)
    if out is None:
        out = torch.empty(B * Ho * Wo, kp, device=x.device, dtype=dtype)
    mean, rstd, gamma, beta = bn if bn is not None else (None,) * 4
    sb, sc, sh, sw = x.stride()
    check(lib.dfm_conv3s2_im2col(dtype_code(x), dtype_code(out), B, H, W, C, sb, sc, sh, sw, ptr(x), ptr(mean),
                                 ptr(rstd), ptr(gamma), ptr(beta), int(gelu), kp, ptr(out), stream()),
          "dfm_conv3s2_im2col")
    if ACCOUNT is not None:
        _acct(0, B * C * H * W * _es(x) + out.numel() * _es(out))
    return out


def conv3s2_col2im(dcols, shape, cin, x=None, bn=None, gelu=False, dx=None, accumulate=False):
    """Backward of conv3s2_im2col w.r.t. the BN output (rows [B*H*W, cin]); x: the rows the gather
    read (needed with gelu, to recompute GELU' of the folded BN output)."""
    B, H, W = shape
    if dx is None:
        dx = torch.empty(B * H * W, cin, device=dcols.device, dtype=dcols.dtype)
        accumulate = False
    mean, rstd, gamma, beta = bn if bn is not None else (None,) * 4
    check(lib.dfm_conv3s2_col2im(dtype_code(dcols), B, H, W, cin, ptr(dcols), ld(dcols), ptr(x),
                                 ld(x) if x is not None else 0, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
                                 int(gelu), ptr(dx), ld(dx), int(accumulate), stream()), "dfm_conv3s2_col2im")
    if ACCOUNT is not None:
        _acct(0, dcols.shape[0] * 9 * cin * _es(dcols) + dx.numel() * _es(dx) * (1 + bool(accumulate) + bool(gelu)))
    return dx


def conv3s2_col2im_nchw(dcols, shape, cin, dtype):
    """Input gradient of a conv with no folded BN: contiguous NCHW [B, cin, H, W] in `dtype`."""
    B, H, W = shape
    dx = torch.empty(B, cin, H, W, device=dcols.device, dtype=dtype)
    sb, sc, sh, sw = dx.stride()
    check(lib.dfm_conv3s2_col2im_nchw(dtype_code(dcols), dtype_code(dx), B, H, W, cin, ptr(dcols), ld(dcols),
                                      ptr(dx), sb, sc, sh, sw, stream()), "dfm_conv3s2_col2im_nchw")
    if ACCOUNT is not None:
        _acct(0, dcols.shape[0] * 9 * cin * _es(dcols) + dx.numel() * _es(dx))
    return dx


def conv3s1_im2col(x, shape, out=None):
    """Gather of nn.Conv2d(cin, cout, 3, 1, 1)'s operand (fcnhead.py:19) from NHWC rows x [B*H*W, cin]
    (cin % 8 == 0): cols [B*H*W, 9*cin] in x.dtype, columns (kh, kw, c) like conv3s2_im2col."""
    B, H, W = shape
    cin = x.shape[1]
    if out is None:
        out = torch.empty(B * H * W, conv3s2_kp(cin), device=x.device, dtype=x.dtype)
    check(lib.dfm_conv3s1_im2col(dtype_code(x), B, H, W, cin, ptr(x), ld(x), ptr(out), ld(out), stream()),
          "dfm_conv3s1_im2col")
    if ACCOUNT is not None:
        _acct(0, B * H * W * cin * _es(x) * (1 + 9))
    return out


def conv3s1_col2im(dcols, shape, cin, dx=None, accumulate=False):
    """Backward of conv3s1_im2col: dx [B*H*W, cin] (+)= the fixed-order sum of every pixel's taps."""
    B, H, W = shape
    if dx is None:
        dx = torch.empty(B * H * W, cin, device=dcols.device, dtype=dcols.dtype)
        accumulate = False
    check(lib.dfm_conv3s1_col2im(dtype_code(dcols), B, H, W, cin, ptr(dcols), ld(dcols), ptr(dx), ld(dx),
                                 int(accumulate), stream()), "dfm_conv3s1_col2im")
    if ACCOUNT is not None:
        _acct(0, B * H * W * cin * _es(dcols) * (9 + 1 + bool(accumulate)))
    return dx


def conv3_weight_pack(w, dtype, kp):
    cout, cin = w.shape[:2]
    out = torch.empty(cout, kp, device=w.device, dtype=dtype)
    check(lib.dfm_conv3_weight_pack(dtype_code(out), cout, cin, kp, ptr(w), ptr(out), stream()),
          "dfm_conv3_weight_pack")
    if ACCOUNT is not None:
        _acct(0, w.numel() * 4 + out.numel() * _es(out))
    return out


def conv3_weight_unpack(dwp, cin, dw=None, accumulate=False):
    cout, kp = dwp.shape
    if dw is None:
        dw = torch.empty(cout, cin, 3, 3, device=dwp.device, dtype=torch.float32)
        accumulate = False
    check(lib.dfm_conv3_weight_unpack(cout, cin, kp, ptr(dwp), ptr(dw), int(accumulate), stream()),
          "dfm_conv3_weight_unpack")
    if ACCOUNT is not None:
        _acct(0, dwp.numel() * 4 + dw.numel() * 4)
    return dw


# ------------------------------------ implicit-GEMM 3x3 conv + pyramid pooling (UPerNet head)
def conv3_igemm_supported(dtype, cin, cout):
    code = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}.get(dtype, -1)
    return bool(lib.dfm_conv3s1_igemm_supported(code, cin, cout))


def conv3_igemm(x, shape, wp, bias=None, out=None, accumulate=False):
    """y [B*H*W, cout] (+)= conv3x3(x, stride 1, pad 1) + bias on NHWC rows x [B*H*W, cin] (a column slice of a
    wider buffer is fine, as is `out`), wp [cout, 9*cin] the packed weight. No gathered operand is formed.
    With the pack of conv3_weight_pack_dgrad and x = dy this is the conv's input gradient."""
    B, H, W = shape
    cin = x.shape[1]
    cout = wp.shape[0]
    assert wp.shape[1] == 9 * cin and wp.is_contiguous() and wp.dtype == x.dtype, (tuple(wp.shape), cin)
    if out is None:
        out = torch.empty(B * H * W, cout, device=x.device, dtype=x.dtype)
        accumulate = False
    check(lib.dfm_conv3s1_igemm_fwd(dtype_code(x), B, H, W, cin, cout, ptr(x), ld(x), ptr(wp), ptr(bias), ptr(out),
                                    ld(out), int(accumulate), stream()), "dfm_conv3s1_igemm_fwd")
    if ACCOUNT is not None:
        P = B * H * W
        _acct(2.0 * P * cout * 9 * cin, _es(x) * (P * cin + P * cout * (1 + bool(accumulate)) + 9 * cin * cout),
              "bf16" if x.dtype != torch.float32 else "f32")
    return out


def conv3_weight_pack_dgrad(w, dtype):
    """[cin, 9*cout] pack of w.permute(1, 0, 2, 3).flip(2, 3): conv3_igemm on dy with it is the input gradient."""
    cout, cin = w.shape[:2]
    out = torch.empty(cin, 9 * cout, device=w.device, dtype=dtype)
    check(lib.dfm_conv3_weight_pack_dgrad(dtype_code(out), cout, cin, ptr(w), ptr(out), stream()),
          "dfm_conv3_weight_pack_dgrad")
    if ACCOUNT is not None:
        _acct(0, w.numel() * 4 + out.numel() * _es(out))
    return out


def conv3_igemm_wgrad(dy, x, shape, bias_grad=False, bias_out=None):
    """dwp [cout, 9*cin] float32 (packed layout, for conv3_weight_unpack) = sum_p dy[p]^T (x) gathered x[p];
    bias_grad=True also db [cout] = sum_p dy[p] (into `bias_out` when given). Split-K over pixels with a
    fixed-order second stage: bit-reproducible."""
    B, H, W = shape
    cin, cout = x.shape[1], dy.shape[1]
    dwp = torch.empty(cout, 9 * cin, device=dy.device, dtype=torch.float32)
    db = None
    if bias_grad:
        db = bias_out if bias_out is not None else torch.empty(cout, device=dy.device, dtype=torch.float32)
    need = lib.dfm_conv3s1_igemm_wgrad_workspace_size(dtype_code(dy), B, H, W, cin, cout, int(bias_grad))
    ws = _ws(need, dy.device)
    check(lib.dfm_conv3s1_igemm_wgrad(dtype_code(dy), B, H, W, cin, cout, ptr(dy), ld(dy), ptr(x), ld(x), ptr(dwp),
                                      ptr(db), ptr(ws), ws.numel() if ws is not None else 0, stream()),
          "dfm_conv3s1_igemm_wgrad")
    if ACCOUNT is not None:
        P = B * H * W
        _acct(2.0 * P * cout * 9 * cin, _es(x) * P * (cin + cout) + 4 * (9 * cin + 1) * cout,
              "bf16" if x.dtype != torch.float32 else "f32")
    return (dwp, db) if bias_grad else dwp


def _scales4(scales):
    s = tuple(int(v) for v in scales)
    assert 1 <= len(s) <= 4, "pyramid pooling takes 1..4 scales"
    return s + (0,) * (4 - len(s))


def ppm_pool(x, shape, scales, out=None):
    """nn.AdaptiveAvgPool2d(s) of NHWC rows x [B*H*W, C] for every s in `scales` in one launch:
    [B * sum s^2, C], scale-major (scale k owns rows [B*off_k, B*off_{k+1}), the NHWC rows of a B x s x s map)."""
    B, H, W = shape
    C = x.shape[1]
    rows = B * sum(s * s for s in scales)
    if out is None:
        out = torch.empty(rows, C, device=x.device, dtype=x.dtype)
    check(lib.dfm_ppm_pool_fwd(dtype_code(x), B, H, W, C, *_scales4(scales), ptr(x), ld(x), ptr(out), ld(out),
                               stream()), "dfm_ppm_pool_fwd")
    if ACCOUNT is not None:
        _acct(0, (B * H * W * len(scales) + rows) * C * _es(x))
    return out


def ppm_pool_bwd(dy, shape, scales, dx=None, accumulate=False):
    B, H, W = shape
    C = dy.shape[1]
    if dx is None:
        dx = torch.empty(B * H * W, C, device=dy.device, dtype=dy.dtype)
        accumulate = False
    check(lib.dfm_ppm_pool_bwd(dtype_code(dy), B, H, W, C, *_scales4(scales), ptr(dy), ld(dy), ptr(dx), ld(dx),
                               int(accumulate), stream()), "dfm_ppm_pool_bwd")
    if ACCOUNT is not None:
        _acct(0, (B * H * W * (1 + bool(accumulate)) + dy.shape[0]) * C * _es(dy))
    return dx


# ------------------------------------------------------------------ multi-scale + flip eval
def resize_nchw(x, size, align_corners, flip=False, dtype=torch.float32):
    """F.interpolate(x, size, 'bilinear', align_corners) [then torch.flip(dims=(3,))], x any strides."""
    B, C, Hi, Wi = x.shape
    Ho, Wo = size
    y = torch.empty(B, C, Ho, Wo, device=x.device, dtype=dtype)
    sb, sc, sh, sw = x.stride()
    check(lib.dfm_resize_nchw(dtype_code(x), dtype_code(y), B, C, Hi, Wi, sb, sc, sh, sw, ptr(x), Ho, Wo,
                              int(align_corners), int(flip), ptr(y), stream()), "dfm_resize_nchw")
    return y


def msf_accumulate(low_rows, B, h, w, ncls, scaled_hw, out_hw, flip, acc):
    """acc [B*H*W, ncls] float32 += softmax(resize_ac(flip?(upsample(low -> scaled_hw))))."""
    (Hs, Ws), (H, W) = scaled_hw, out_hw
    check(lib.dfm_msf_accumulate(dtype_code(low_rows), B, h, w, ncls, ptr(low_rows), ld(low_rows), Hs, Ws, H, W,
                                 int(flip), ptr(acc), stream()), "dfm_msf_accumulate")
    return acc


def slide_grids(n, crop, stride):
    """val_mm.py:295-296: the number of sliding windows along an axis of n pixels."""
    return max(n - crop + stride - 1, 0) // stride + 1


def slide_msf_accumulate(low_rows, B, h, w, ncls, crop_hw, stride_hw, scaled_hw, out_hw, flip, acc, softmax=True):
    """msf_accumulate over sliding windows: low_rows [G*B*h*w, ncls] holds the low-res logits of the
    G = hg*wg windows (window-major) of crop_hw pixels that cover the scaled_hw image at stride_hw; the
    scaled logits are their per-pixel average (val_mm.py:257-322). softmax=False stores the averaged
    logits, resized to out_hw, into acc instead of adding their softmax."""
    (hc, wc), (hs, ws), (Hs, Ws), (H, W) = crop_hw, stride_hw, scaled_hw, out_hw
    if hs > 0 and ws > 0:  # the library rejects the rest; the buffers' sizes are only known here
        G = slide_grids(Hs, hc, hs) * slide_grids(Ws, wc, ws)
        if low_rows.dim() != 2 or low_rows.shape[0] < G * B * h * w or low_rows.shape[1] < ncls:
            raise ValueError(f"slide_msf_accumulate: low rows {tuple(low_rows.shape)} do not hold {G} windows x "
                             f"{B} x {h} x {w} x {ncls}")
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() != B * H * W * ncls:
        raise ValueError(f"slide_msf_accumulate: acc {tuple(acc.shape)} {acc.dtype} is not contiguous float32 "
                         f"[{B}*{H}*{W}, {ncls}]")
    check(lib.dfm_slide_msf_accumulate(dtype_code(low_rows), B, h, w, ncls, ptr(low_rows), ld(low_rows), hc, wc, hs,
                                       ws, Hs, Ws, H, W, int(flip), int(softmax), ptr(acc), stream()),
          "dfm_slide_msf_accumulate")
    return acc


def seg_confusion(acc, label, ncls, ignore, hist):
    """hist [ncls*ncls] int64 += bincount(label*ncls + argmax(acc rows)) over label != ignore."""
    assert label.dtype == torch.int64 and hist.dtype == torch.int64 and acc.is_contiguous()
    assert label.is_contiguous()
    if acc.dim() != 2 or acc.shape[1] != ncls or acc.shape[0] != label.numel():
        raise ValueError(f"seg_confusion: scores {tuple(acc.shape)} do not match {label.numel()} labels x {ncls}")
    check(lib.dfm_seg_confusion(label.numel(), ncls, ptr(acc), ptr(label), ignore, ptr(hist), stream()),
          "dfm_seg_confusion")
    return hist


def seg_predict(low_rows, B, h, w, ncls, out_hw, pred=None, label=None, ignore=255, hist=None):
    """argmax over classes of the align_corners=False upsampling of the low-res logits low_rows
    [B*h*w, >= ncls] to out_hw, without materialising it (builder.py:203 + val_mm.py:129-132).
    pred: uint8 [B, H, W] to fill; None allocates it, unless a label is given: then only the histogram
    is computed. With label [B, H, W] int64, hist [ncls*ncls] int64 += bincount(label*ncls + argmax)
    over label != ignore. Returns pred (hist when there is no pred)."""
    H, W = out_hw
    if low_rows.dim() != 2 or low_rows.shape[0] < B * h * w or low_rows.shape[1] < ncls:
        raise ValueError(f"seg_predict: low rows {tuple(low_rows.shape)} do not hold {B} x {h} x {w} x {ncls}")
    if (label is None) != (hist is None):
        raise ValueError("seg_predict: label and hist go together")
    if label is not None:
        if label.dtype != torch.int64 or not label.is_contiguous() or label.numel() != B * H * W:
            raise ValueError(f"seg_predict: label {tuple(label.shape)} {label.dtype} is not contiguous int64 "
                             f"[{B}, {H}, {W}]")
        if hist.dtype != torch.int64 or not hist.is_contiguous() or hist.numel() != ncls * ncls:
            raise ValueError(f"seg_predict: hist {tuple(hist.shape)} {hist.dtype} is not contiguous int64 "
                             f"[{ncls}*{ncls}]")
    if pred is None and label is None:
        pred = torch.empty(B, H, W, device=low_rows.device, dtype=torch.uint8)
    if pred is not None and (pred.dtype != torch.uint8 or not pred.is_contiguous() or pred.numel() != B * H * W):
        raise ValueError(f"seg_predict: pred {tuple(pred.shape)} {pred.dtype} is not contiguous uint8 [{B}, {H}, {W}]")
    check(lib.dfm_seg_predict(dtype_code(low_rows), B, h, w, ncls, ptr(low_rows), ld(low_rows), H, W, ptr(pred),
                              ptr(label), ignore, ptr(hist), stream()), "dfm_seg_predict")
    if ACCOUNT is not None:
        npix = B * H * W
        _acct(0, B * h * w * ncls * _es(low_rows) + npix * ((pred is not None) + 8 * (label is not None)))
    return pred if pred is not None else hist


def rows_argmax(acc, ncls, out=None):
    """uint8 [rows] = argmax over the ncls float32 scores of each row of acc (first maximum)."""
    if acc.dim() != 2 or acc.shape[1] != ncls or acc.dtype != torch.float32 or not acc.is_contiguous():
        raise ValueError(f"rows_argmax: scores {tuple(acc.shape)} {acc.dtype} are not contiguous float32 [*, {ncls}]")
    if out is None:
        out = torch.empty(acc.shape[0], device=acc.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != acc.shape[0]:
        raise ValueError(f"rows_argmax: out {tuple(out.shape)} {out.dtype} is not contiguous uint8 [{acc.shape[0]}]")
    check(lib.dfm_rows_argmax(acc.shape[0], ncls, ptr(acc), ptr(out), stream()), "dfm_rows_argmax")
    if ACCOUNT is not None:
        _acct(0, acc.numel() * 4 + acc.shape[0])
    return out


# ------------------------------------------------------------------- laser-scan expansion (Trav)
LASER_MAX_N = 8192  # DFM_LASER_MAX_N: the ranges of one scan a workgroup stages in LDS


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} {tuple(t.shape)} {t.dtype} is not contiguous float32")
    return t


def laser_expand_fwd(x, alpha, g, c, Hout, save=True):
    """The collapsed Attention1Dto2D (DFormer.py:308-339): scans x [B, N], alpha [L, Hh], g [Hh], c [1]
    (float32) -> (plane [B, Hout, L], s [B, L], mean, var [B, L, Hh]); mean / var are None unless save."""
    B, N = x.shape
    L, Hh = alpha.shape
    for t, what in ((x, "laser_expand_fwd: scans"), (alpha, "laser_expand_fwd: alpha"), (g, "laser_expand_fwd: g"),
                    (c, "laser_expand_fwd: c")):
        _f32c(t, what)
    if g.numel() != Hh or c.numel() != 1:
        raise ValueError(f"laser_expand_fwd: g {tuple(g.shape)} / c {tuple(c.shape)} do not match {Hh} heads")
    s = torch.empty(B, L, device=x.device, dtype=torch.float32)
    plane = torch.empty(B, Hout, L, device=x.device, dtype=torch.float32)
    mean = torch.empty(B, L, Hh, device=x.device, dtype=torch.float32) if save else None
    var = torch.empty_like(mean) if save else None
    check(lib.dfm_laser_expand_fwd(B, N, L, Hh, Hout, ptr(x), ptr(alpha), ptr(g), ptr(c), ptr(s), ptr(mean), ptr(var),
                                   ptr(plane), stream()), "dfm_laser_expand_fwd")
    if ACCOUNT is not None:  # per (b, l, h, j): sub, mul, exp, add, fma (+ the variance walk's sub, mul, exp, mul, fma)
        _acct(B * L * Hh * N * (6.0 + 6.0 * save),
              4 * (B * N + L * Hh + Hh + 1 + B * L + B * Hout * L + 2 * save * B * L * Hh), "f32")
    return plane, s, mean, var


def laser_expand_bwd(dplane, g, mean, var):
    """dplane [B, Hout, L] -> (ds [B, L], dalpha [L, Hh], dg [Hh], dc [1]), fixed-order sums."""
    B, Hout, L = dplane.shape
    Hh = g.numel()
    for t, what in ((dplane, "laser_expand_bwd: dplane"), (g, "laser_expand_bwd: g"), (mean, "laser_expand_bwd: mean"),
                    (var, "laser_expand_bwd: var")):
        _f32c(t, what)
    if tuple(mean.shape) != (B, L, Hh) or tuple(var.shape) != (B, L, Hh):
        raise ValueError(f"laser_expand_bwd: moments {tuple(mean.shape)} / {tuple(var.shape)} are not [{B}, {L}, {Hh}]")
    dev = dplane.device
    ds = torch.empty(B, L, device=dev, dtype=torch.float32)
    dalpha = torch.empty(L, Hh, device=dev, dtype=torch.float32)
    dg = torch.empty(Hh, device=dev, dtype=torch.float32)
    dc = torch.empty(1, device=dev, dtype=torch.float32)
    ws = _ws(lib.dfm_laser_expand_bwd_workspace(L, Hh), dev)
    check(lib.dfm_laser_expand_bwd(B, L, Hh, Hout, ptr(dplane), ptr(g), ptr(mean), ptr(var), ptr(ds), ptr(dalpha),
                                   ptr(dg), ptr(dc), ptr(ws), stream()), "dfm_laser_expand_bwd")
    if ACCOUNT is not None:
        _acct(B * Hout * L + 4.0 * B * L * Hh + B * L,
              4 * (B * Hout * L + B * L + 2 * B * L * Hh + L * Hh + 2 * Hh + 1), "f32")
    return ds, dalpha, dg, dc


# ---------------------------------------------------------------------------------------- NMF
def _copy_dtype(flag):
    """bf16_copy argument: False / None (no copy), True (bf16) or a 16-bit torch dtype."""
    if not flag:
        return None
    return torch.bfloat16 if flag is True else flag


def nmf_update(a, num, den, eps=1e-6, out=None, bf16_copy=False):
    """out = a * num / (den + eps) (float32); with bf16_copy (True = bf16, or a 16-bit dtype) also
    returns a 16-bit copy of out."""
    if out is None:
        out = torch.empty_like(a)
    cdt = _copy_dtype(bf16_copy)
    o16 = torch.empty(a.shape, device=a.device, dtype=cdt) if cdt is not None else None
    check(lib.dfm_nmf_update(a.numel(), ptr(a), ptr(num), ptr(den), eps, ptr(out), ptr(o16),
                             dtype_code(o16) if o16 is not None else 0, stream()), "dfm_nmf_update")
    if ACCOUNT is not None:
        _acct(0, a.numel() * (16 + 2 * bool(bf16_copy)))
    return (out, o16) if bf16_copy else out


def nmf_update_bwd(g, a, num, den, out, ga=None, accumulate=False, eps=1e-6, bf16_copy=False):
    """-> ga, gnum, gden (float32) [, bf16 copy of gnum]."""
    if ga is None:
        ga = torch.empty_like(a)
        accumulate = False
    gnum = torch.empty_like(a)
    gden = torch.empty_like(a)
    cdt = _copy_dtype(bf16_copy)
    g16 = torch.empty(a.shape, device=a.device, dtype=cdt) if cdt is not None else None
    check(lib.dfm_nmf_update_bwd(a.numel(), ptr(g), ptr(a), ptr(num), ptr(den), ptr(out), eps, ptr(ga),
                                 int(accumulate), ptr(gnum), ptr(gden), ptr(g16),
                                 dtype_code(g16) if g16 is not None else 0, stream()), "dfm_nmf_update_bwd")
    if ACCOUNT is not None:
        _acct(0, a.numel() * (4 * (8 + bool(accumulate)) + 2 * bool(bf16_copy)))
    return (ga, gnum, gden, g16) if bf16_copy else (ga, gnum, gden)


def nmf_update_mm(a, num, M, eps=1e-6, bf16_copy=False):
    """Batched [B, rows, 64] update with its denominator product fused: den = a M, out = a * num /
    (den + eps). Returns (out, den[, 16-bit copy of out])."""
    Bb, rows, R = a.shape
    out, den = torch.empty_like(a), torch.empty_like(a)
    cdt = _copy_dtype(bf16_copy)
    o16 = torch.empty(a.shape, device=a.device, dtype=cdt) if cdt is not None else None
    check(lib.dfm_nmf_update_mm(Bb, rows, R, ptr(a), ptr(num), ptr(M), eps, ptr(den), ptr(out), ptr(o16),
                                dtype_code(o16) if o16 is not None else 0, stream()), "dfm_nmf_update_mm")
    if ACCOUNT is not None:
        _acct(2.0 * a.numel() * R, a.numel() * (16 + 2 * bool(bf16_copy)) + M.numel() * 4)
    return (out, den, o16) if bf16_copy else (out, den)


def nmf_update_bwd_mm(g, a, num, den, out, A2=None, S=None, Mg=None, eps=1e-6, bf16_copy=False):
    """Backward of nmf_update_mm with g' = g + A2 (S + S^T) and ga = g' num / (den+eps) + gden Mg.
    Returns (ga, gnum, gden[, 16-bit copy of gnum])."""
    Bb, rows, R = a.shape
    ga, gnum, gden = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    cdt = _copy_dtype(bf16_copy)
    g16 = torch.empty(a.shape, device=a.device, dtype=cdt) if cdt is not None else None
    check(lib.dfm_nmf_update_bwd_mm(Bb, rows, R, ptr(g), ptr(A2), ptr(S), ptr(a), ptr(num), ptr(den), ptr(out), eps,
                                    ptr(Mg), ptr(ga), 0, ptr(gnum), ptr(gden), ptr(g16),
                                    dtype_code(g16) if g16 is not None else 0, stream()), "dfm_nmf_update_bwd_mm")
    if ACCOUNT is not None:
        _acct(2.0 * a.numel() * R * ((A2 is not None) + (Mg is not None)),
              a.numel() * (4 * (8 + (A2 is not None)) + 2 * bool(bf16_copy)))
    return (ga, gnum, gden, g16) if bf16_copy else (ga, gnum, gden)


def nmf_fwd(x, bases, steps, eps=1e-6, keep=False):
    """NMF2D forward in one library call (dfm_nmf_fwd): x [B, N, D], bases [B, D, 64] float32 -> y
    [B, N, D]; keep=True also returns the saved factors for nmf_bwd (a uint8 buffer)."""
    Bb, N, D = x.shape
    R = bases.shape[2]
    assert x.is_contiguous() and bases.is_contiguous() and bases.dtype == torch.float32
    dt = dtype_code(x)
    nbytes = lib.dfm_nmf_fwd_workspace_size(dt, Bb, N, D, R, steps)
    assert nbytes > 0, "dfm_nmf_fwd: unsupported shape / rank"
    saved = None
    if keep:
        sb = lib.dfm_nmf_saved_size(dt, Bb, N, D, R, steps)
        saved = torch.empty(sb, device=x.device, dtype=torch.uint8)
    ws = _ws(nbytes, x.device)
    y = torch.empty_like(x)
    check(lib.dfm_nmf_fwd(dt, Bb, N, D, R, steps, eps, ptr(x), ptr(bases), ptr(y), ptr(saved),
                          saved.numel() if keep else 0, ptr(ws), nbytes, stream()), "dfm_nmf_fwd")
    return (y, saved) if keep else y


def nmf_bwd(x, bases, saved, gy, steps, eps=1e-6):
    """Gradient of nmf_fwd's y w.r.t. x (dfm_nmf_bwd) from the factors nmf_fwd(keep=True) saved."""
    Bb, N, D = x.shape
    R = bases.shape[2]
    assert gy.is_contiguous() and gy.dtype == x.dtype
    dt = dtype_code(x)
    nbytes = lib.dfm_nmf_bwd_workspace_size(dt, Bb, N, D, R, steps)
    ws = _ws(nbytes, x.device)
    gx = torch.empty_like(x)
    check(lib.dfm_nmf_bwd(dt, Bb, N, D, R, steps, eps, ptr(x), ptr(bases), ptr(saved), saved.numel(), ptr(gy),
                          ptr(gx), ptr(ws), nbytes, stream()), "dfm_nmf_bwd")
    return gx


def softmax_rows(x):
    y = torch.empty_like(x)
    check(lib.dfm_softmax_rows(x.numel() // x.shape[-1], x.shape[-1], ptr(x), ptr(y), stream()), "dfm_softmax_rows")
    if ACCOUNT is not None:
        _acct(0, x.numel() * 8)
    return y


def softmax_rows_bwd(y, dy, dx=None, accumulate=False):
    if dx is None:
        dx = torch.empty_like(y)
        accumulate = False
    check(lib.dfm_softmax_rows_bwd(y.numel() // y.shape[-1], y.shape[-1], ptr(y), ptr(dy), ptr(dx), int(accumulate),
                                   stream()), "dfm_softmax_rows_bwd")
    if ACCOUNT is not None:
        _acct(0, y.numel() * 4 * (3 + bool(accumulate)))
    return dx


# --------------------------------------------------------------------------------------- loss
def seg_loss_fwd(logits, B, h, w, ncls, label, ignore=255):
    H, W = label.shape[-2:]
    out = torch.empty(2, device=logits.device, dtype=torch.float32)
    ws = _ws(lib.dfm_seg_loss_workspace(B, H, W), logits.device)
    check(lib.dfm_seg_loss_fwd(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore, None,
                               ptr(out), ptr(ws), stream()), "dfm_seg_loss_fwd")
    if ACCOUNT is not None:
        _acct(0, logits.numel() * _es(logits) + label.numel() * 8)
    return out


def seg_loss_bwd(logits, B, h, w, ncls, label, loss_out, gscale=None, ignore=255):
    H, W = label.shape[-2:]
    dl = torch.empty(B * h * w, ncls, device=logits.device, dtype=torch.float32)
    ws = _ws(lib.dfm_seg_loss_bwd_workspace(B, h, w, ncls, H, W), logits.device)
    check(lib.dfm_seg_loss_bwd(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore, None,
                               ptr(loss_out), ptr(gscale), ptr(dl), ptr(ws), stream()), "dfm_seg_loss_bwd")
    if ACCOUNT is not None:
        _acct(0, logits.numel() * (_es(logits) + 4) + label.numel() * 8)
    return dl


def seg_loss_grad_partials_size(B, h, w, ncls, H, W):
    return lib.dfm_seg_loss_grad_partials_size(B, h, w, ncls, H, W)


def seg_loss_fwd_grad(logits, B, h, w, ncls, label, ignore=255):
    """Training loss + its gradient's unscaled per-tile partials in one pass -> (loss_out, partials)."""
    H, W = label.shape[-2:]
    out = torch.empty(2, device=logits.device, dtype=torch.float32)
    nb = seg_loss_grad_partials_size(B, h, w, ncls, H, W)
    part = torch.empty(nb // 4, device=logits.device, dtype=torch.float32)
    check(lib.dfm_seg_loss_fwd_grad(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                    ptr(out), ptr(part), stream()), "dfm_seg_loss_fwd_grad")
    if ACCOUNT is not None:
        _acct(0, logits.numel() * _es(logits) + label.numel() * 8)
    return out, part


def seg_loss_bwd_gather(part, B, h, w, ncls, loss_out, gscale, dtype):
    dl = torch.empty(B * h * w, ncls, device=part.device, dtype=dtype)
    check(lib.dfm_seg_loss_bwd_gather(dtype_code(dl), B, h, w, ncls, ptr(part), ptr(loss_out), ptr(gscale), ptr(dl),
                                      stream()), "dfm_seg_loss_bwd_gather")
    if ACCOUNT is not None:
        _acct(0, dl.numel() * _es(dl))
    return dl


def _seg_loss_args(what, logits, B, h, w, ncls, label, weight):
    """The buffer checks the criterion-option wrappers share; returns the label size (H, W)."""
    if logits.dim() != 2 or not logits.is_contiguous() or tuple(logits.shape) != (B * h * w, ncls):
        raise ValueError(f"{what}: logits {tuple(logits.shape)} are not contiguous [{B}*{h}*{w}, {ncls}]")
    if label.dtype != torch.int64 or not label.is_contiguous() or label.dim() != 3 or label.shape[0] != B:
        raise ValueError(f"{what}: label {tuple(label.shape)} {label.dtype} is not contiguous int64 [{B}, H, W]")
    if weight is not None and (weight.dtype != torch.float32 or not weight.is_contiguous() or
                               weight.numel() != ncls or weight.device != logits.device):
        raise ValueError(f"{what}: weight {tuple(weight.shape)} {weight.dtype} on {weight.device} is not contiguous "
                         f"float32 [{ncls}] on {logits.device}")
    return tuple(label.shape[-2:])


def seg_loss_opts_fwd(logits, B, h, w, ncls, label, weight=None, label_smoothing=0.0, ignore=255):
    """seg_loss_fwd with class weights (float32 [ncls] or None) and label smoothing -> (sum, valid count)."""
    H, W = _seg_loss_args("seg_loss_opts_fwd", logits, B, h, w, ncls, label, weight)
    out = torch.empty(2, device=logits.device, dtype=torch.float32)
    ws = _ws(lib.dfm_seg_loss_workspace(B, H, W), logits.device)
    check(lib.dfm_seg_loss_opts_fwd(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                    ptr(weight), label_smoothing, ptr(out), ptr(ws), stream()),
          "dfm_seg_loss_opts_fwd")
    if ACCOUNT is not None:
        _acct(0, logits.numel() * _es(logits) + label.numel() * 8)
    return out


def seg_loss_opts_bwd(logits, B, h, w, ncls, label, loss_out, weight=None, label_smoothing=0.0, gscale=None,
                      ignore=255):
    H, W = _seg_loss_args("seg_loss_opts_bwd", logits, B, h, w, ncls, label, weight)
    if loss_out.dtype != torch.float32 or loss_out.numel() != 2:
        raise ValueError(f"seg_loss_opts_bwd: loss_out {tuple(loss_out.shape)} {loss_out.dtype} is not float32 [2]")
    dl = torch.empty(B * h * w, ncls, device=logits.device, dtype=torch.float32)
    ws = _ws(lib.dfm_seg_loss_bwd_workspace(B, h, w, ncls, H, W), logits.device)
    check(lib.dfm_seg_loss_opts_bwd(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                    ptr(weight), label_smoothing, ptr(loss_out), ptr(gscale), ptr(dl), ptr(ws),
                                    stream()), "dfm_seg_loss_opts_bwd")
    if ACCOUNT is not None:
        _acct(0, logits.numel() * (_es(logits) + 4) + label.numel() * 8)
    return dl


def seg_loss_opts_fwd_grad(logits, B, h, w, ncls, label, weight=None, label_smoothing=0.0, ignore=255):
    """seg_loss_fwd_grad with class weights and label smoothing -> (loss_out, partials for seg_loss_bwd_gather)."""
    H, W = _seg_loss_args("seg_loss_opts_fwd_grad", logits, B, h, w, ncls, label, weight)
    nb = seg_loss_grad_partials_size(B, h, w, ncls, H, W)
    if nb == 0:
        raise ValueError(f"seg_loss_opts_fwd_grad: ({h}, {w}) -> ({H}, {W}) is not an upsampling by 4 or 8")
    out = torch.empty(2, device=logits.device, dtype=torch.float32)
    part = torch.empty(nb // 4, device=logits.device, dtype=torch.float32)
    check(lib.dfm_seg_loss_opts_fwd_grad(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                         ptr(weight), label_smoothing, ptr(out), ptr(part), stream()),
          "dfm_seg_loss_opts_fwd_grad")
    if ACCOUNT is not None:
        _acct(0, logits.numel() * _es(logits) + label.numel() * 8)
    return out, part


def seg_loss_ohem_relabel(logits, B, h, w, ncls, label, thresh, min_kept, ignore=255):
    """Online hard example mining as label rewriting (loss_opr.py:157-185), all on the device:
    -> (label_out int64 like label, prob float32 like label, stats float32 [2] = (threshold, num_valid))."""
    H, W = _seg_loss_args("seg_loss_ohem_relabel", logits, B, h, w, ncls, label, None)
    if not 0.0 <= thresh <= 1.0 or min_kept < 0:
        raise ValueError(f"seg_loss_ohem_relabel: thresh {thresh} not in [0, 1] or min_kept {min_kept} negative")
    prob = torch.empty(B, H, W, device=logits.device, dtype=torch.float32)
    out = torch.empty_like(label)
    stats = torch.empty(2, device=logits.device, dtype=torch.float32)
    ws = _ws(lib.dfm_seg_loss_ohem_workspace(B, H, W), logits.device)
    check(lib.dfm_seg_loss_ohem_relabel(dtype_code(logits), B, h, w, ncls, ptr(logits), H, W, ptr(label), ignore,
                                        float(thresh), int(min_kept), ptr(prob), ptr(out), ptr(stats), ptr(ws),
                                        stream()), "dfm_seg_loss_ohem_relabel")
    if ACCOUNT is not None:  # the prob plane is written once and read by 3 select passes and the relabel
        _acct(0, logits.numel() * _es(logits) + label.numel() * (8 + 4 + 4 * 4 + 8))
    return out, prob, stats


# ------------------------------------------------------------- few-shot episodes (meta_forward)
def fss_mask_footprint(mask, low_hw):
    """int64 masks [n, H, W] -> (foot [n, 2, h', w'], count [n, 2]) float32: the adjoint of the bilinear
    upsample (h', w') -> (H, W) applied to the indicators of classes 0 and 1, and their pixel counts."""
    n, H, W = mask.shape
    hs, ws = low_hw
    if mask.dtype != torch.int64 or not mask.is_contiguous():
        raise ValueError(f"fss_mask_footprint: masks {tuple(mask.shape)} {mask.dtype} are not contiguous int64")
    foot = torch.empty(n, 2, hs, ws, device=mask.device, dtype=torch.float32)
    count = torch.empty(n, 2, device=mask.device, dtype=torch.float32)
    ws_ = _ws(lib.dfm_fss_footprint_workspace(n, hs, ws, H, W), mask.device)
    check(lib.dfm_fss_mask_footprint(n, hs, ws, H, W, ptr(mask), ptr(foot), ptr(count), ptr(ws_), stream()),
          "dfm_fss_mask_footprint")
    if ACCOUNT is not None:  # per pixel and class: one compare and two tap multiply-adds per pass
        _acct(8.0 * n * H * W, 8 * n * H * W + 4 * (foot.numel() + count.numel()), "f32")
    return foot, count


def fss_proto_pool_fwd(f, foot, count, B, S):
    """Support rows f [B*S*cells, C] (row stride ld(f)) -> (proto [B, 2, C] float32, wgt [B*S*cells, 2])."""
    rows, C = f.shape
    cells = rows // (B * S)
    assert rows == B * S * cells and foot.numel() == 2 * rows and count.numel() == 2 * B * S
    wgt = torch.empty(rows, 2, device=f.device, dtype=torch.float32)
    proto = torch.empty(B, 2, C, device=f.device, dtype=torch.float32)
    check(lib.dfm_fss_proto_pool_fwd(dtype_code(f), B, S, cells, C, ptr(f), ld(f), ptr(_f32c(foot, "fss foot")),
                                     ptr(_f32c(count, "fss count")), ptr(wgt), ptr(proto), stream()),
          "dfm_fss_proto_pool_fwd")
    if ACCOUNT is not None:
        _acct(4.0 * rows * C, rows * C * _es(f) + 4 * (4 * rows + 2 * B * S + 2 * B * C), "f32")
    return proto, wgt


def fss_proto_pool_bwd(wgt, dproto, B, S, dtype, out=None):
    """df [B*S*cells, C] (dtype; `out` when given) = wgt[:, 0] x dproto[b, 0] + wgt[:, 1] x dproto[b, 1]."""
    rows, C = wgt.shape[0], dproto.shape[-1]
    df = torch.empty(rows, C, device=wgt.device, dtype=dtype) if out is None else out
    assert df.dtype == dtype and tuple(df.shape) == (rows, C)
    check(lib.dfm_fss_proto_pool_bwd(dtype_code(df), B, S, rows // (B * S), C, ptr(wgt),
                                     ptr(_f32c(dproto, "fss dproto")), ptr(df), ld(df), stream()),
          "dfm_fss_proto_pool_bwd")
    if ACCOUNT is not None:
        _acct(3.0 * rows * C, rows * C * _es(df) + 4 * (2 * rows + 2 * B * C), "f32")
    return df


def fss_sim_fwd(q, proto, temperature=1.0, save=True):
    """Query rows q [B*cells, C], proto [B, 2, C] -> (prob [B*cells, 2], saved): softmax over [bg, fg] of
    20 cos(q, proto) / temperature; saved = (cos, qnorm, pnorm) for fss_sim_bwd (cos / qnorm None unless save)."""
    rows, C = q.shape
    B = proto.shape[0]
    cells = rows // B
    assert rows == B * cells and tuple(proto.shape) == (B, 2, C)
    dev = q.device
    prob = torch.empty(rows, 2, device=dev, dtype=torch.float32)
    cosv = torch.empty(rows, 2, device=dev, dtype=torch.float32) if save else None
    qnorm = torch.empty(rows, device=dev, dtype=torch.float32) if save else None
    pnorm = torch.empty(B, 2, device=dev, dtype=torch.float32)
    check(lib.dfm_fss_sim_fwd(dtype_code(q), B, cells, C, ptr(q), ld(q), ptr(_f32c(proto, "fss proto")),
                              1.0 / temperature, ptr(prob), ptr(cosv), ptr(qnorm), ptr(pnorm), stream()),
          "dfm_fss_sim_fwd")
    if ACCOUNT is not None:
        _acct(6.0 * rows * C, rows * C * _es(q) + 4 * (2 * B * C + rows * (2 + 3 * save) + 2 * B), "f32")
    return prob, (cosv, qnorm, pnorm)


def fss_sim_bwd(q, proto, dprob, prob, saved, temperature=1.0, dq=None, accumulate=False):
    """(dq [B*cells, C] in q's dtype (+= into dq when accumulate), dproto [B, 2, C] float32)."""
    rows, C = q.shape
    B = proto.shape[0]
    cosv, qnorm, pnorm = saved
    if dq is None:
        dq = torch.empty(rows, C, device=q.device, dtype=q.dtype)
        accumulate = False
    assert dq.dtype == q.dtype
    dproto = torch.empty(B, 2, C, device=q.device, dtype=torch.float32)
    ws = _ws(lib.dfm_fss_sim_bwd_workspace(B, rows // B), q.device)
    check(lib.dfm_fss_sim_bwd(dtype_code(q), B, rows // B, C, ptr(q), ld(q), ptr(proto), 1.0 / temperature,
                              ptr(_f32c(dprob, "fss dprob")), ptr(prob), ptr(cosv), ptr(qnorm), ptr(pnorm), ptr(dq),
                              ld(dq), int(accumulate), ptr(dproto), ptr(ws), stream()), "dfm_fss_sim_bwd")
    if ACCOUNT is not None:  # q is read by both the row sum and the outer product
        _acct(10.0 * rows * C, rows * C * _es(q) * (3 + bool(accumulate)) + 4 * (4 * B * C + 7 * rows), "f32")
    return dq, dproto


def fss_loss_fwd(low, B, h, w, prob, hs, ws, label, alpha, save=True):
    """low [B*h*w, >= 2] decode-head logits rows, prob [B*hs*ws, 2] float32, label int64 [B, H, W] ->
    (loss_out = (sum, count), gplane [B, H, W] float32 or None): CE of alpha up(low) + (1 - alpha) up(prob)
    over the pixels labelled 0 or 1."""
    H, W = label.shape[-2:]
    out = torch.empty(2, device=low.device, dtype=torch.float32)
    gplane = torch.empty(B, H, W, device=low.device, dtype=torch.float32) if save else None
    wsp = _ws(lib.dfm_fss_loss_workspace(), low.device)
    check(lib.dfm_fss_loss_fwd(dtype_code(low), B, h, w, ptr(low), ld(low), hs, ws, ptr(_f32c(prob, "fss prob")), H, W,
                               ptr(label), float(alpha), ptr(gplane), ptr(out), ptr(wsp), stream()), "dfm_fss_loss_fwd")
    if ACCOUNT is not None:
        _acct(0, B * h * w * 2 * _es(low) + prob.numel() * 4 + label.numel() * (8 + 4 * save))
    return out, gplane


def fss_loss_bwd(gplane, B, h, w, hs, ws, loss_out, alpha, dtype, gscale=None):
    """(dlow [B*h*w, 2] in dtype, dprob [B*hs*ws, 2] float32) from the forward's residual plane."""
    H, W = gplane.shape[-2:]
    dlow = torch.empty(B * h * w, 2, device=gplane.device, dtype=dtype)
    dprob = torch.empty(B * hs * ws, 2, device=gplane.device, dtype=torch.float32)
    wsp = _ws(lib.dfm_fss_loss_bwd_workspace(B, h, w, hs, ws, H, W), gplane.device)
    check(lib.dfm_fss_loss_bwd(dtype_code(dlow), B, h, w, hs, ws, H, W, ptr(gplane), ptr(loss_out), ptr(gscale),
                               float(alpha), ptr(dlow), ptr(dprob), ptr(wsp), stream()), "dfm_fss_loss_bwd")
    if ACCOUNT is not None:  # the plane is read once per grid
        _acct(0, 2 * gplane.numel() * 4 + dlow.numel() * _es(dlow) + dprob.numel() * 4)
    return dlow, dprob


def fss_fuse(low, B, h, w, prob, hs, ws, out_hw, alpha):
    """The fused full-resolution logits alpha up(low) + (1 - alpha) up(prob): float32 [B*H*W, 2] rows."""
    H, W = out_hw
    out = torch.empty(B * H * W, 2, device=low.device, dtype=torch.float32)
    check(lib.dfm_fss_fuse_fwd(dtype_code(low), B, h, w, ptr(low), ld(low), hs, ws, ptr(_f32c(prob, "fss prob")), H, W,
                               float(alpha), ptr(out), stream()), "dfm_fss_fuse_fwd")
    if ACCOUNT is not None:
        _acct(0, B * h * w * 2 * _es(low) + prob.numel() * 4 + out.numel() * 4)
    return out


# -------------------------------------------------------------------------------------- optimizer
def _f32_flat(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"dformer_amd: {what} must be a contiguous float32 buffer")
    return t


def _win(win):
    """The window state {micro_index, accum_steps}: int32 [2] on the device, or None."""
    if win is not None and (win.dtype != torch.int32 or win.numel() < 2):
        raise ValueError("dformer_amd: win is int32 [2]")
    return ptr(win)


def loss_scale_update(amp, flag, growth, backoff, interval, win=None):
    """GradScaler.update on the device state; inside an accumulation window (`win`) the scaler is left alone."""
    check(lib.dfm_loss_scale_update_win(ptr(amp), ptr(flag), growth, backoff, interval, _win(win), stream()),
          "dfm_loss_scale_update_win")


def grad_nonfinite(g, flag):
    """flag (int32 [1], zeroed by the caller) := 1 if any element of g is inf / nan."""
    check(lib.dfm_grad_nonfinite(g.numel(), ptr(g), ptr(flag), stream()), "dfm_grad_nonfinite")
    return flag


def adamw(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, bf16_copy=None, hyper=None,
          amp=None, flag=None, clip_state=None, win=None, ema=None, ema_decay=0.0, clear_g=False):
    """AdamW step; with `hyper` (device float32 [lr, step]) lr and step are read on the device
    (lr / step arguments ignored) so the launch can live in a replayed HIP graph. With the loss
    scaler's device state `amp` and overflow `flag` the step is skipped / unscaled on the device.
    The options need `hyper` and are off when None: the gradient times clip_state[1]; no write
    unless `win` (int32 {micro_index, accum_steps}) is on its last micro-step; `ema` updated in the
    same pass; clear_g zeroes g (the accumulation buffer)."""
    n = p.numel()
    for t, what in ((g, "g"), (m, "m"), (v, "v"), (ema, "ema"), (bf16_copy, "bf16_copy")):
        if t is not None and t.numel() != n:
            raise ValueError(f"adamw: {what} has {t.numel()} elements, p has {n}")
    cdt = dtype_code(bf16_copy) if bf16_copy is not None else 0
    bufs = [ptr(_f32_flat(t, what)) for t, what in ((p, "p"), (g, "g"), (m, "m"), (v, "v"))]
    if hyper is not None:
        check(lib.dfm_adamw_opt(n, bufs[0], bufs[1], int(clear_g), bufs[2], bufs[3], ptr(hyper), ptr(amp), ptr(flag),
                                ptr(clip_state), _win(win), ptr(None if ema is None else _f32_flat(ema, "ema")),
                                ema_decay, beta1, beta2, eps, weight_decay, grad_scale, ptr(bf16_copy), cdt, stream()),
              "dfm_adamw_opt")
    else:
        if any(o is not None for o in (amp, flag, clip_state, win, ema)) or clear_g:
            raise ValueError("adamw: amp / flag and the options need hyper")
        check(lib.dfm_adamw(n, *bufs, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ptr(bf16_copy), cdt,
                            stream()), "dfm_adamw")
    if ACCOUNT is not None:
        _acct(0, n * (28 + (2 if bf16_copy is not None else 0) + (8 if ema is not None else 0)
                      + (4 if clear_g else 0)))


def grad_accumulate(acc, g):
    """acc += g over flat float32 buffers (p.grad += g of a backward without zero_grad())."""
    if acc.numel() != g.numel():
        raise ValueError(f"grad_accumulate: {acc.numel()} vs {g.numel()} elements")
    check(lib.dfm_grad_accumulate(acc.numel(), ptr(_f32_flat(acc, "acc")), ptr(_f32_flat(g, "g")), stream()),
          "dfm_grad_accumulate")
    if ACCOUNT is not None:
        _acct(0, acc.numel() * 12)


def sumsq_blocks():
    """Partials dfm_grad_sumsq writes per buffer."""
    return lib.dfm_grad_sumsq_blocks()


def grad_sumsq(g, part, flag=None, win=None):
    """Stage one of the global gradient norm: sumsq_blocks() float32 partials of sum g^2 into `part`
    (this buffer's slice of the partial buffer); with `flag` also grad_nonfinite over the same read."""
    if part.numel() < sumsq_blocks():
        raise ValueError(f"grad_sumsq: {part.numel()} partial slots, {sumsq_blocks()} needed")
    check(lib.dfm_grad_sumsq(g.numel(), ptr(_f32_flat(g, "g")), ptr(_f32_flat(part, "part")), ptr(flag), _win(win),
                             stream()), "dfm_grad_sumsq")
    if ACCOUNT is not None:
        _acct(0, g.numel() * 4)


def grad_clip_coef(part, grad_scale, max_norm, clip_state, amp=None, win=None):
    """Stage two over the partials of every buffer: clip_state (float32 [2]) = {total_norm, coef} of
    torch.nn.utils.clip_grad_norm_(max_norm) for gradients g * grad_scale (/ the loss scale amp[0])."""
    if clip_state.numel() < 2 or clip_state.dtype != torch.float32:
        raise ValueError("grad_clip_coef: clip_state is float32 [2]")
    check(lib.dfm_grad_clip_coef(part.numel(), ptr(_f32_flat(part, "part")), grad_scale, ptr(amp), max_norm,
                                 ptr(clip_state), _win(win), stream()), "dfm_grad_clip_coef")
    if ACCOUNT is not None:
        _acct(0, part.numel() * 4)
