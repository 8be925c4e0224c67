"""The ConvFFN backward's route through dfm_ffn_dgrad_dw3_bwd (functional.FFN_DGRAD_DW3_MIN_ROWS = 0, so the
small golden planes take it): Block goldens, a graphed-versus-eager step, and proof that the kernel ran (GPU)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KERNEL = "ffn_dgrad_dw3_kernel"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def traced(fn):
    """Run fn with the launch tracer on; returns (fn's result, names of the kernels the wrappers launched)."""
    from dformer_amd import kernels as Kk
    Kk.ACCOUNT = []
    Kk.trace(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        Kk.trace(0)
        acct, Kk.ACCOUNT = Kk.ACCOUNT, None
    return out, [Kk.kernel_name(f) for a in acct for f in a[0]]


@pytest.mark.parametrize("name", ["block_base_s0", "block_base_s1", "block_tiny_s1"])
def test_block_bf16_goldens_on_the_fused_route(name, monkeypatch):
    """The gates of test_block_gpu.test_block_bf16_vs_reference_goldens (4 x the reference's own bf16 envelope)
    with both ConvFFN backwards of the Block on the fused kernel; a silent fallback to the pair fails."""
    from dformer_amd import functional as Fn
    from test_block_gpu import bf16_envelope_check, run_block
    monkeypatch.setattr(Fn, "FFN_DGRAD_DW3_MIN_ROWS", 0)
    monkeypatch.setattr(Fn, "FUSED_FFN", "auto")
    (g, blk, x, xe, y, ye, last), names = traced(lambda: run_block(name, torch.bfloat16))
    assert sum(KERNEL in n for n in names) == 2, names  # RGB and depth ConvFFN
    assert not any("dw3_rows_bwd_kernel" in n or "dw3_stream_bwd_kernel" in n for n in names), names
    grads = {k: p.grad for k, p in blk.named_parameters() if p.grad is not None}
    bf16_envelope_check(name, "ffn-dgrad-dw3", g, y, ye, x.grad, xe.grad, grads, last)


def test_graphed_steps_match_eager_on_the_fused_route(monkeypatch):
    """test_graph_gpu.test_graphed_steps_match_eager's pattern (DFormer-Tiny + ham, 2 x 240 x 320) with every
    supported ConvFFN backward on the fused kernel: eager and graph replay agree bit for bit."""
    import bench
    from dformer_amd import functional as Fn
    from dformer_amd.train import FusedAdamW, GraphedTrainStep, train_step
    from test_graph_gpu import _build
    monkeypatch.setattr(Fn, "FFN_DGRAD_DW3_MIN_ROWS", 0)
    det, bm = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        dev = torch.device("cuda", 0)
        cfg, ma = _build("ham")
        _, mb = _build("ham")
        ma = ma.to(dev).set_compute_dtype(torch.bfloat16)
        mb = mb.to(dev).set_compute_dtype(torch.bfloat16)
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        bases = torch.rand(2, 512, 64, device=dev, generator=gen)
        bases = bases / bases.norm(dim=1, keepdim=True)
        for m in (ma, mb):
            m.decode_head.hamburger.ham.injected_bases = bases
            m.return_logits = False
            m.train()
        oa = FusedAdamW(ma, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
        ob = FusedAdamW(mb, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
        rgb, dep, lab = bench.synthetic_batch(2, 240, 320, cfg.num_classes, dev, 5)
        first, names = traced(lambda: train_step(ma, oa, rgb, dep, lab).item())
        assert sum(KERNEL in n for n in names) > 0, sorted(set(names))
        la = [first] + [train_step(ma, oa, rgb, dep, lab).item() for _ in range(4)]
        g = GraphedTrainStep(mb, ob, rgb, dep, lab, warmup=2)
        lb = [g().item() for _ in range(3)]
        assert ob.step_count == oa.step_count == 5
        assert la[2:] == lb, (la, lb)
        for ga, gb in zip(oa.groups, ob.groups):
            assert torch.equal(ga.flat, gb.flat) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det, bm
