"""FusedAdamW's options on the GPU: gradient accumulation, clipping by the global gradient norm and
the weight EMA, at the kernel level (flat buffers against torch) and at the step level (DFormer-Tiny
+ ham, 2 x 64x96, bf16; torch.optim.AdamW / clip_grad_norm_ / lerp_ are the references).

Measured figures are printed before they are asserted (pytest -s shows them); DESIGN.md 6h quotes them."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [1, 255, 256, 257, 70_001, 3_000_001]  # one element, a block edge, an odd grid tail, several grid strides
B1, B2, EPS, LR, WD = 0.9, 0.999, 1e-8, 1e-3, 0.01
ULP = 2.0 ** -24  # one fp32 rounding, relative


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    det, bm = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det, bm


def _dev():
    return torch.device("cuda", 0)


def _randn(n, seed, scale=1.0):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return torch.randn(n, device=_dev(), generator=g) * scale


def _norm_tol(x):
    """Allowed relative error of a norm of x: 4 x what torch's own fp32 vector_norm shows against
    fp64 on the same data (the summation orders differ), floor 1e-6. Returns (fp64 norm, tolerance)."""
    ref = torch.linalg.vector_norm(x.double()).item()
    terr = abs(torch.linalg.vector_norm(x).item() - ref) / ref
    return ref, max(4 * terr, 1e-6), terr


def _norm(K, bufs, gscale=1.0, max_norm=1e30, amp=None, flag=None, win=None, clip=None):
    nb = K.sumsq_blocks()
    part = torch.zeros(len(bufs) * nb, device=_dev())
    clip = torch.zeros(2, device=_dev()) if clip is None else clip
    for j, b in enumerate(bufs):
        K.grad_sumsq(b, part[j * nb:(j + 1) * nb], flag=flag, win=win)
    K.grad_clip_coef(part, gscale, max_norm, clip, amp=amp, win=win)
    return clip, part


# ================================================================================= kernel level: norm
@pytest.mark.parametrize("n", SIZES)
def test_norm_matches_fp64_and_repeats(n):
    from dformer_amd import kernels as K
    x = _randn(n, 100 + n % 97, 3.0)
    ref, tol, terr = _norm_tol(x)
    clip, part = _norm(K, [x])
    clip2, part2 = _norm(K, [x])
    err = abs(clip[0].item() - ref) / ref
    print(f"norm n={n}: rel err {err:.3e} (torch fp32 {terr:.3e}, allowed {tol:.3e})")
    assert err <= tol, (err, tol)
    assert torch.equal(clip, clip2) and torch.equal(part, part2)  # bit-reproducible
    assert clip[1].item() == 1.0  # max_norm above the norm: no clipping
    # clip_grad_norm_'s coefficient when it clips, and the scale factors of the fp16 path
    amp = torch.tensor([1024.0, 0.0, 0.0, 0.0], device=_dev())
    c3, _ = _norm(K, [x], gscale=0.25, max_norm=0.5 * ref * 0.25 / 1024.0, amp=amp)
    want = ref * 0.25 / 1024.0
    assert abs(c3[0].item() - want) / want <= tol
    coef = torch.tensor(0.5 * want, dtype=torch.float32) / (c3[0].cpu() + 1e-6)
    assert abs(c3[1].item() - coef.item()) <= 2 * ULP * coef.item() and c3[1].item() < 1.0
    if n > 1:  # a buffer that is not 16-byte aligned takes the scalar path
        y = x[1:]
        refy, toly, _ = _norm_tol(y)
        cy, _ = _norm(K, [y])
        assert abs(cy[0].item() - refy) / refy <= toly


def test_norm_two_groups_one_norm():
    from dformer_amd import kernels as K
    a, b = _randn(70_001, 1, 2.0), _randn(257, 2, 5.0)
    ref, tol, _ = _norm_tol(torch.cat([a, b]))
    clip, _ = _norm(K, [a, b])
    assert abs(clip[0].item() - ref) / ref <= tol
    ca, _ = _norm(K, [a])
    assert clip[0].item() > ca[0].item()


@pytest.mark.parametrize("bad,where", [(float("nan"), 0), (float("inf"), -1), (float("-inf"), 40_000)])
def test_norm_nonfinite_propagates(bad, where):
    from dformer_amd import kernels as K
    x = _randn(70_001, 3)
    flag = torch.zeros(1, device=_dev(), dtype=torch.int32)
    _norm(K, [x], max_norm=1.0, flag=flag)
    assert flag.item() == 0  # clean gradients leave the flag alone
    x[where] = bad
    clip, _ = _norm(K, [x], max_norm=1.0, flag=flag)
    assert flag.item() == 1
    assert not np.isfinite(clip[0].item())
    # clip_grad_norm_: nan norm -> nan coefficient, inf norm -> coefficient 0
    if np.isnan(bad):
        assert np.isnan(clip[0].item()) and np.isnan(clip[1].item())
    else:
        assert clip[0].item() == float("inf") and clip[1].item() == 0.0


def test_norm_waits_for_the_last_micro_step():
    from dformer_amd import kernels as K
    x = _randn(70_001, 4)
    win = torch.tensor([0, 2], device=_dev(), dtype=torch.int32)
    flag = torch.zeros(1, device=_dev(), dtype=torch.int32)
    x[5] = float("inf")
    clip = torch.full((2,), -7.0, device=_dev())
    clip, part = _norm(K, [x], max_norm=1.0, flag=flag, win=win, clip=clip)
    assert clip.tolist() == [-7.0, -7.0] and not part.any() and flag.item() == 0
    win[0] = 1
    clip, part = _norm(K, [x], max_norm=1.0, flag=flag, win=win, clip=clip)
    assert clip[0].item() == float("inf") and flag.item() == 1


# ========================================================================== kernel level: accumulate
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_is_fp32_add(n):
    from dformer_amd import kernels as K
    acc, g = _randn(n + 1, 5, 2.0), _randn(n + 1, 6)
    want = acc + g
    K.grad_accumulate(acc[:n], g[:n])
    assert torch.equal(acc[:n], want[:n]) and acc[n].item() != want[n].item()  # nothing past n
    acc2 = _randn(n + 1, 5, 2.0)
    K.grad_accumulate(acc2[1:], g[1:])  # 4-byte aligned only: the scalar path
    assert torch.equal(acc2[1:], want[1:]) and acc2[0].item() != want[0].item()


# ============================================================================ kernel level: update
class _Bufs:
    """p, m, v, 16-bit copy (and the option buffers) of one run, from fixed seeds."""

    def __init__(self, n, copy_dtype=torch.bfloat16):
        self.p = _randn(n, 7)
        self.m = torch.zeros(n, device=_dev())
        self.v = torch.zeros(n, device=_dev())
        self.copy = torch.zeros(n, device=_dev(), dtype=copy_dtype)
        self.ema = self.p.clone()
        self.hyper = torch.tensor([LR, 1.0], device=_dev())

    def all(self):
        return (self.p, self.m, self.v, self.copy)

    def same(self, other):
        return all(torch.equal(a, b) for a, b in zip(self.all(), other.all()))


def _grads(n, steps=3):
    return [_randn(n, 20 + t, 0.3) for t in range(steps)]


def _adamw(K, b, g, gscale, opt, **kw):
    """K.adamw(hyper=...) on the buffers b, asserting with the launch tracer which instantiation of the
    one update kernel ran: without this a dispatch slip would compare a kernel with itself."""
    import kernel_variants as kv
    with kv.Trace() as tr:
        K.adamw(b.p, g, b.m, b.v, 0.0, B1, B2, EPS, WD, 1, gscale, b.copy, hyper=b.hyper, **kw)
    tc = {torch.bfloat16: "unsigned short", torch.float16: "f16_t"}[b.copy.dtype]
    assert tr.launched == [f"adamw_kernel<{tc}, {'true' if opt else 'false'}>"], tr.launched


@pytest.mark.parametrize("n", SIZES)
def test_update_variant_bit_relations(n):
    from dformer_amd import kernels as K
    gs = _grads(n)
    ref, one = _Bufs(n), _Bufs(n)
    clip1 = torch.tensor([5.0, 1.0], device=_dev())
    for t, g in enumerate(gs):
        for b in (ref, one):
            b.hyper[1] = float(t + 1)
        _adamw(K, ref, g, 0.5, opt=False)
        _adamw(K, one, g.clone(), 0.5, opt=True, clip_state=clip1)
        assert ref.same(one), f"coef = 1 on the option kernel differs from the plain kernel at step {t + 1}"
    # inside a window: nothing is written; on its last micro-step: the update, and acc cleared
    win = torch.tensor([0, 2], device=_dev(), dtype=torch.int32)
    w = _Bufs(n)
    acc = gs[0].clone()
    _adamw(K, w, acc, 0.5, opt=True, win=win, ema=w.ema, ema_decay=0.9, clear_g=True)
    fresh = _Bufs(n)
    assert w.same(fresh) and torch.equal(w.ema, fresh.ema) and torch.equal(acc, gs[0])
    win[0] = 1
    _adamw(K, w, acc, 0.5, opt=True, win=win, ema=w.ema, ema_decay=0.9, clear_g=True)
    _adamw(K, fresh, gs[0], 0.5, opt=False)
    assert w.same(fresh) and not acc.any()
    assert not torch.equal(w.ema, fresh.ema)  # the average moved with the applied step


@pytest.mark.parametrize("n", [257, 70_001])
def test_update_variant_bit_equal_to_amp(n):
    from dformer_amd import kernels as K
    gs = [g * 1024.0 for g in _grads(n)]
    ref, opt = _Bufs(n, torch.float16), _Bufs(n, torch.float16)
    st = [torch.tensor([1024.0, 0.0, 0.0, 0.0], device=_dev()) for _ in range(2)]
    fl = [torch.zeros(1, device=_dev(), dtype=torch.int32) for _ in range(2)]
    clip1 = torch.tensor([5.0, 1.0], device=_dev())
    win1 = torch.tensor([0, 1], device=_dev(), dtype=torch.int32)  # a window of one micro-step: always its last
    for t, g in enumerate(gs):
        _adamw(K, ref, g, 1.0, opt=False, amp=st[0], flag=fl[0])
        K.loss_scale_update(st[0], fl[0], 2.0, 0.5, 2)
        _adamw(K, opt, g.clone(), 1.0, opt=True, amp=st[1], flag=fl[1], clip_state=clip1)
        K.loss_scale_update(st[1], fl[1], 2.0, 0.5, 2, win=win1)
        assert ref.same(opt), f"step {t + 1}"
        assert torch.equal(st[0], st[1])
    assert st[0].tolist() == [2048.0, 1.0, 3.0, 0.0]  # grew once (interval 2), three applied steps


def _raw_adamw(b, g, amp=None, flag=None, opt=False):
    """dfm_adamw_dev / dfm_adamw_amp (no wrapper of the package calls them any more; they stay in
    the ABI) or the dfm_adamw_opt call that stands for them, through the library directly."""
    from dformer_amd import _lib
    from dformer_amd._lib import dtype_code, ptr, stream
    lib, tail = _lib.lib, (B1, B2, EPS, WD, 0.5, ptr(b.copy), dtype_code(b.copy), stream())
    bufs = (b.p.numel(), ptr(b.p), ptr(g), ptr(b.m), ptr(b.v), ptr(b.hyper))
    if opt:
        st = lib.dfm_adamw_opt(*bufs[:3], 0, *bufs[3:], ptr(amp), ptr(flag), None, None, None, 0.0, *tail)
    elif amp is not None:
        st = lib.dfm_adamw_amp(*bufs, ptr(amp), ptr(flag), *tail)
    else:
        st = lib.dfm_adamw_dev(*bufs, *tail)
    _lib.check(st, "raw adamw")


@pytest.mark.parametrize("copy_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", [257, 70_001])
def test_abi_entry_points_give_the_wrapper_bits(n, copy_dtype):
    """dfm_adamw_dev and dfm_adamw_amp against dfm_adamw_opt with the same arguments, 3 steps."""
    amp = torch.tensor([4.0, 0.0, 0.0, 0.0], device=_dev())
    flag = torch.zeros(1, device=_dev(), dtype=torch.int32)
    dev, dev_opt, hal, hal_opt = (_Bufs(n, copy_dtype) for _ in range(4))
    for t, g in enumerate(_grads(n)):
        for b in (dev, dev_opt, hal, hal_opt):
            b.hyper[1] = float(t + 1)
        amp[2] = float(t)  # applied steps so far: the amp path's step count is amp[2] + 1
        _raw_adamw(dev, g)
        _raw_adamw(dev_opt, g, opt=True)
        _raw_adamw(hal, g * 4.0, amp, flag)
        _raw_adamw(hal_opt, g * 4.0, amp, flag, opt=True)
        assert dev.same(dev_opt), f"dfm_adamw_dev, step {t + 1}"
        assert hal.same(hal_opt), f"dfm_adamw_amp, step {t + 1}"
    assert not dev.same(_Bufs(n, copy_dtype)) and not hal.same(_Bufs(n, copy_dtype))  # the updates were applied
    assert torch.equal(dev.p, hal.p)  # g * 4 unscaled by amp[0] = 4 is g, exactly


def _err(x, x64):
    return ((x.double() - x64).abs().max() / x64.abs().max()).item()


@pytest.mark.parametrize("n", [257, 70_001])
def test_update_variant_against_fp64_torch(n):
    """clip_grad_norm_ + torch.optim.AdamW in fp64 on the same gradients for 3 steps, plus the
    ema.lerp_ recursion. The plain kernel (fed the fp64-clipped gradients rounded to fp32) is
    measured against the same trajectory; the option kernel, which clips by itself, stays within 2 x
    its error: the arithmetic is identical up to one extra multiply."""
    from dformer_amd import kernels as K
    gs = _grads(n)
    max_norm, d = 0.25 * torch.linalg.vector_norm(gs[0].double()).item(), 0.9
    old, new = _Bufs(n), _Bufs(n)
    p64 = torch.nn.Parameter(old.p.double().clone())
    ema64 = p64.detach().clone()
    topt = torch.optim.AdamW([p64], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    for t, g in enumerate(gs):
        p64.grad = g.double().clone()
        total = torch.nn.utils.clip_grad_norm_([p64], max_norm)
        assert total.item() > max_norm  # the clip is active
        topt.step()
        ema64.lerp_(p64.detach(), 1 - d)
        for b in (old, new):
            b.hyper[1] = float(t + 1)
        _adamw(K, old, p64.grad.float(), 1.0, opt=False)
        clip, _ = _norm(K, [g], max_norm=max_norm)
        _adamw(K, new, g.clone(), 1.0, opt=True, clip_state=clip, ema=new.ema, ema_decay=d)
    st = topt.state[p64]
    for name, xo, xn, x64 in (("p", old.p, new.p, p64.detach()), ("m", old.m, new.m, st["exp_avg"]),
                              ("v", old.v, new.v, st["exp_avg_sq"])):
        eo, en = _err(xo, x64), _err(xn, x64)
        print(f"update n={n} {name}: plain {eo:.3e}, with options {en:.3e}")
        assert en <= 2 * eo, (name, en, eo)
    # the average: a convex combination of the p trajectory (error <= p's) plus, per step, the
    # roundings of d, 1 - d, the product and the fused add
    ee, ep = _err(new.ema, ema64), _err(new.p, p64.detach())
    print(f"update n={n} ema: {ee:.3e} (p {ep:.3e})")
    assert ee <= ep + 3 * 4 * ULP, (ee, ep)


# ========================================================================= kernel level: fp16 scaler
def _window(K, bufs, acc, grads, win, st, fl, clip, poison=None):
    """One accumulation window at the kernel level, the launches FusedAdamW issues per micro-step."""
    for i, g in enumerate(grads):
        win[0] = i
        K.grad_accumulate(acc, g)
        if poison == ("flag", i):
            fl.fill_(1)
        _norm(K, [acc], gscale=1.0 / len(grads), max_norm=1.0, amp=st, flag=fl, win=win, clip=clip)
        _adamw(K, bufs, acc, 1.0 / len(grads), opt=True, amp=st, flag=fl, clip_state=clip, win=win, ema=bufs.ema,
               ema_decay=0.9, clear_g=True)
        K.loss_scale_update(st, fl, 2.0, 0.5, 2000, win)


@pytest.mark.parametrize("how", ["inf_grad", "flag"])
def test_fp16_overflow_skips_the_window(how):
    from dformer_amd import kernels as K
    n, k = 70_001, 3
    b, fresh = _Bufs(n, torch.float16), _Bufs(n, torch.float16)
    acc = torch.zeros(n, device=_dev())
    st = torch.tensor([65536.0, 5.0, 0.0, 0.0], device=_dev())
    fl = torch.zeros(1, device=_dev(), dtype=torch.int32)
    win = torch.tensor([0, k], device=_dev(), dtype=torch.int32)
    clip = torch.zeros(2, device=_dev())
    grads = [g * 65536.0 for g in _grads(n, k)]
    if how == "inf_grad":
        grads[1][n // 2] = float("inf")
    _window(K, b, acc, grads, win, st, fl, clip, poison=("flag", 1) if how == "flag" else None)
    assert b.same(fresh) and torch.equal(b.ema, fresh.ema)  # no parameter, moment or average moved
    assert not acc.any()                                    # the skipped update still cleared acc
    assert st.tolist() == [32768.0, 0.0, 0.0, 1.0] and fl.item() == 0  # one backoff, skipped + 1
    # a clean window of k micro-steps: one applied step, growth_tracker + 1 (not + k), scale untouched
    _window(K, b, acc, [g * 32768.0 for g in _grads(n, k)], win, st, fl, clip)
    assert st.tolist() == [32768.0, 1.0, 1.0, 1.0] and fl.item() == 0
    assert not b.same(fresh) and not acc.any() and torch.isfinite(b.p).all()
    assert 0.0 < clip[1].item() < 1.0  # the norm was taken on the unscaled mean gradient


# ======================================================================================= step level
def _make(syncbn=False, dtype=torch.bfloat16):
    import bench
    from dformer_amd.segmentor import EncoderDecoder
    cfg = bench.make_cfg("DFormer-Tiny", "ham")
    cfg["drop_path_rate"] = 0.0
    torch.manual_seed(3)
    m = EncoderDecoder(cfg=cfg, syncbn=syncbn)
    m.decode_head.dropout_ratio = 0.0
    m = m.to(_dev()).set_compute_dtype(dtype)
    g = torch.Generator(device=_dev()).manual_seed(11)
    bases = torch.rand(2, 512, 64, device=_dev(), generator=g)
    m.decode_head.hamburger.ham.injected_bases = bases / bases.norm(dim=1, keepdim=True)
    m.return_logits = False
    return cfg, m.train()


def _opt(model, dtype=torch.bfloat16, lr=LR, **kw):
    from dformer_amd.train import FusedAdamW
    return FusedAdamW(model, lr=lr, weight_decay=WD, compute_dtype=dtype, **kw)


def _batch(seed):
    import bench
    return bench.synthetic_batch(2, 64, 96, 40, _dev(), seed)


def _snap(opt):
    return [(g.flat.clone(), g.m.clone(), g.v.clone()) for g in opt.groups]


def _same(snap, opt):
    return all(torch.equal(a, b) for s, g in zip(snap, opt.groups) for a, b in zip(s, (g.flat, g.m, g.v)))


@pytest.fixture(scope="module")
def plain(_gpu):
    """The step as it was: FusedAdamW(model) on batch 5, its state after each of 3 steps."""
    from dformer_amd.train import train_step
    _, m = _make()
    opt = _opt(m)
    flat0 = [g.flat.clone() for g in opt.groups]
    snaps, losses = [], []
    for _ in range(3):
        losses.append(train_step(m, opt, *_batch(5)).item())
        snaps.append(_snap(opt))
    assert all(g.acc is None and g.ema is None for g in opt.groups)  # no option buffer exists
    assert opt.win is None and opt.clip_state is None and opt.partials is None
    return dict(flat0=flat0, snaps=snaps, losses=losses)


@pytest.fixture(scope="module")
def twin(_gpu):
    """A twin model stepped at lr = 0 (its parameters never move): the flat gradients of batches 5
    and 6 at the initial weights, and which slots got a gradient at all."""
    from dformer_amd.train import train_step
    _, m = _make()
    opt = _opt(m, lr=0.0)
    flat0 = [g.flat.clone() for g in opt.groups]
    grads = []
    for seed in (5, 6):
        train_step(m, opt, *_batch(seed))
        grads.append([g.grad.clone() for g in opt.groups])
    fired = [torch.ones_like(g.flat, dtype=torch.bool) for g in opt.groups]
    for g, off, k in opt.buckets.unfired:
        fired[opt.groups.index(g)][off:off + k] = False
    assert all(torch.equal(a, g.flat) for a, g in zip(flat0, opt.groups))
    return dict(grads=grads, fired=fired, wds=[g.wd for g in opt.groups])


def _torch_adamw(flat0, grads, wds):
    """One torch.optim.AdamW fp32 step over the two flat buffers."""
    ps = [torch.nn.Parameter(f.clone()) for f in flat0]
    topt = torch.optim.AdamW([dict(params=[p], weight_decay=wd) for p, wd in zip(ps, wds)], lr=LR, betas=(B1, B2),
                             eps=EPS)
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    topt.step()
    return [p.detach() for p in ps]


def test_defaults_are_the_plain_step(plain):
    from dformer_amd.train import train_step
    _, m = _make()
    opt = _opt(m, accum_steps=1, max_grad_norm=None, ema_decay=None)
    losses = [train_step(m, opt, *_batch(5)).item() for _ in range(3)]
    assert losses == plain["losses"] and _same(plain["snaps"][2], opt) and opt.step_count == 3
    assert not opt.options and all(g.acc is None and g.ema is None for g in opt.groups)
    assert opt.win is None and opt.clip_state is None and opt.partials is None


def test_accumulating_one_batch_twice_is_the_plain_step(plain):
    """g + g is exact in fp32 and grad_scale is 1/2: bit-equal to the plain step on that batch."""
    from dformer_amd.train import train_step
    _, m = _make()
    opt = _opt(m, accum_steps=2)
    for w in range(2):
        for i in range(2):
            before = _snap(opt)
            loss = train_step(m, opt, *_batch(5)).item()
            assert loss == plain["losses"][w]  # each call returns its micro-batch's mean loss
            if i == 0:
                assert _same(before, opt) and opt.step_count == w  # nothing moves inside the window
        assert _same(plain["snaps"][w], opt), f"window {w}"
        assert all(not g.acc.any() for g in opt.groups)
    assert opt.step_count == 2


def test_accumulating_two_batches_matches_torch_adamw(plain, twin):
    from dformer_amd.train import train_step
    _, m = _make()
    opt = _opt(m, accum_steps=2)
    for seed in (5, 6):
        train_step(m, opt, *_batch(seed))
    g1, g2 = twin["grads"]
    mean = [(a + b) / 2 for a, b in zip(g1, g2)]
    want = _torch_adamw(plain["flat0"], mean, twin["wds"])
    base = _torch_adamw(plain["flat0"], g1, twin["wds"])
    # parameters without a gradient are left alone here and decayed by a torch AdamW fed zeros: the
    # comparison is over the slots that got one
    e_acc = max((g.flat - w)[f].abs().max().item() for g, w, f in zip(opt.groups, want, twin["fired"]))
    e_plain = max((s[0] - w)[f].abs().max().item() for s, w, f in zip(plain["snaps"][0], base, twin["fired"]))
    print(f"accumulate step: max abs err {e_acc:.3e} (plain step vs torch AdamW {e_plain:.3e})")
    assert e_acc <= 4 * e_plain, (e_acc, e_plain)
    moved = max((g.flat - f0).abs().max().item() for g, f0 in zip(opt.groups, plain["flat0"]))
    assert moved > 100 * e_acc  # the bound is far below the update itself
    assert opt.step_count == 1


def test_clipping(plain, twin):
    from dformer_amd.train import train_step
    _, m = _make()
    opt = _opt(m, max_grad_norm=1e30)
    for _ in range(2):
        train_step(m, opt, *_batch(5))
    assert _same(plain["snaps"][1], opt)  # a bound never reached is bit-equal to no clipping
    ref2, tol2, _ = _norm_tol(torch.cat([g.grad for g in opt.groups]))  # the second step's gradient, still in its slots
    assert abs(opt.grad_norm() - ref2) / ref2 <= tol2
    ref, tol, terr = _norm_tol(torch.cat(twin["grads"][0]))
    _, m2 = _make()
    half = _opt(m2, max_grad_norm=0.5 * ref)
    train_step(m2, half, *_batch(5))
    err = abs(half.grad_norm() - ref) / ref
    print(f"step grad norm {ref:.6f}: rel err {err:.3e} (torch fp32 {terr:.3e}, allowed {tol:.3e})")
    assert err <= tol
    # coef = max_norm / (norm + 1e-6): the norm's error (tol) and three roundings (max_norm to fp32, the
    # add, the divide). First step: m = (1 - beta1) * g * coef, three more (g * coef, the product with
    # 1 - beta1, itself taken in fp32 as the kernel does, and the fused add of beta1 * 0)
    coef = 0.5 * ref / (ref + 1e-6)
    omb = float(np.float32(1.0) - np.float32(B1))
    assert abs(half.clip_state[1].item() - coef) <= (tol + 3 * ULP) * coef
    for g, gr in zip(half.groups, twin["grads"][0]):
        want = gr.double() * coef * omb
        assert ((g.m.double() - want).abs() <= (tol + 6 * ULP) * want.abs() + 1e-38).all()


def test_ema_recursion_and_eval_on_the_average():
    from dformer_amd.train import train_step
    d = 0.9
    _, m = _make()
    opt = _opt(m, ema_decay=d)
    traj = [[g.flat.double().clone() for g in opt.groups]]
    for _ in range(3):
        train_step(m, opt, *_batch(5))
        traj.append([g.flat.double().clone() for g in opt.groups])
    d32, omd = float(np.float32(d)), float(np.float32(1.0) - np.float32(d))  # the kernel's fp32 constants
    for j, g in enumerate(opt.groups):
        e = traj[0][j].clone()
        big = e.abs()
        for t in range(1, 4):
            e = d32 * e + omd * traj[t][j]
            big = torch.maximum(big, traj[t][j].abs())
        # per step two roundings (the product, the fused add) of values bounded by `big`
        assert ((g.ema.double() - e).abs() <= 3 * 2 * ULP * big + 1e-38).all()
        assert not torch.equal(g.ema, g.flat)
    # evaluation on the averaged weights == a second model loaded from ema_state_dict
    rgb, dep, _ = _batch(7)
    before = [(g.flat.clone(), g.ema.clone(), g.flat.clone() if g.shadow is None else g.shadow.clone())
              for g in opt.groups]
    m.eval()
    with torch.no_grad():
        live = m.predict(rgb, dep)
        with opt.ema_weights():
            avg = m.predict(rgb, dep)
        live2 = m.predict(rgb, dep)
    for (p0, e0, s0), g in zip(before, opt.groups):
        assert torch.equal(g.flat, p0) and torch.equal(g.ema, e0)
        assert torch.equal(g.flat if g.shadow is None else g.shadow, s0)
    assert torch.equal(live, live2)
    _, m2 = _make()
    m2.load_state_dict(opt.ema_state_dict(m))
    m2.eval()
    with torch.no_grad():
        assert torch.equal(m2.predict(rgb, dep), avg)


def _all_on(model, dtype=torch.bfloat16, **kw):
    return _opt(model, dtype, accum_steps=2, max_grad_norm=kw.pop("max_grad_norm", 1.0), ema_decay=0.99, **kw)


def test_graphed_windows_match_eager(twin):
    """All three options: 2 windows eager against 2 windows of replays of one captured graph."""
    from dformer_amd.train import GraphedTrainStep, train_step
    clip_at = 0.5 * torch.linalg.vector_norm(torch.cat(twin["grads"][0]).double()).item()  # clipping is active
    (_, ma), (_, mb) = _make(), _make()
    oa, ob = _all_on(ma, max_grad_norm=clip_at), _all_on(mb, max_grad_norm=clip_at)
    rgb, dep, lab = _batch(5)
    la = [train_step(ma, oa, rgb, dep, lab).item() for _ in range(6)]  # the helper's warm-up window + 2 windows
    g = GraphedTrainStep(mb, ob, rgb, dep, lab, warmup=2)
    lb = []
    for i in range(4):
        before = _snap(ob)
        lb.append(g().item())
        assert _same(before, ob) == (i % 2 == 0)  # the same graph: only every second replay updates
    assert la[2:] == lb, (la, lb)
    assert oa.step_count == ob.step_count == 3
    for ga, gb in zip(oa.groups, ob.groups):
        for a, b in ((ga.flat, gb.flat), (ga.m, gb.m), (ga.v, gb.v), (ga.ema, gb.ema), (ga.acc, gb.acc)):
            assert torch.equal(a, b)
        assert not gb.acc.any()
    assert torch.equal(oa.clip_state, ob.clip_state) and 0.0 < ob.clip_state[1].item() < 1.0


def test_fp16_windows_count_once():
    """The fp16 path with every option, eagerly: each window is one scaler decision."""
    from dformer_amd.train import train_step
    _, m = _make(dtype=torch.float16)
    opt = _all_on(m, torch.float16)
    start = _snap(opt)
    for _ in range(4):
        train_step(m, opt, *_batch(5))
    sc = opt.scaler
    applied, skipped = opt.step_count, sc.skipped
    assert applied + skipped == 2, (applied, skipped)
    assert sc.scale == 65536.0 * 0.5 ** skipped
    assert all(not g.acc.any() for g in opt.groups) and int(sc.found_inf.item()) == 0
    assert _same(start, opt) == (applied == 0)
    assert all(torch.isfinite(g.flat).all() and torch.isfinite(g.ema).all() for g in opt.groups)


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_forced_collectives_one_rank_accumulate():
    """accum_steps = 2 through the world > 1 code with one rank (a 1-rank RCCL group and
    batchnorm.FORCE_COLLECTIVES, as tests/test_graph_gpu.py::test_forced_collectives_one_rank_nccl):
    every micro-step all-reduces its buckets, and the result is bit-equal to no collectives."""
    import torch.distributed as dist
    from dformer_amd import batchnorm as D
    from dformer_amd.train import train_step
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=_dev())
    D.FORCE_COLLECTIVES = True
    try:
        (_, ma), (_, mc) = _make(syncbn=True), _make()
        oa, oc = _all_on(ma, world=1), _all_on(mc, world=1)
        calls = [0]
        real = dist.all_reduce

        def counting(*a, **k):
            calls[0] += 1
            return real(*a, **k)
        dist.all_reduce = counting
        try:
            la = [train_step(ma, oa, *_batch(5 + i % 2)).item() for i in range(4)]
        finally:
            dist.all_reduce = real
        assert calls[0] > 0
        D.FORCE_COLLECTIVES = False
        lc = [train_step(mc, oc, *_batch(5 + i % 2)).item() for i in range(4)]
        assert la == lc, (la, lc)
        assert oa.step_count == oc.step_count == 2
        for ga, gc in zip(oa.groups, oc.groups):
            for a, c in ((ga.flat, gc.flat), (ga.m, gc.m), (ga.v, gc.v), (ga.ema, gc.ema)):
                assert torch.equal(a, c)
        assert torch.equal(oa.clip_state, oc.clip_state)
    except BaseException as e:  # report before the process-group teardown (which may abort on failure)
        print("forced-collectives accumulate failure:", repr(e)[:2000], flush=True)
        raise
    finally:
        D.FORCE_COLLECTIVES = False
        D._GLOBAL_ROWS.clear()
        D._GLOBAL_TOTAL.clear()
        dist.destroy_process_group()
