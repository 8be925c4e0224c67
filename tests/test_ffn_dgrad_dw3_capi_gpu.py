"""The C-ABI Block's route through dfm_ffn_dgrad_dw3_bwd (csrc/block.cpp ffn_chain_bwd): its row threshold is a
compile-time 65,536, so the Block goldens (at most 19,200 rows) never reach it. A stage-0 DFormer-B Block at
4 x 120 x 160 = 76,800 rows does, through dfm_block_fwd / dfm_block_bwd alone, and is compared with the Python
autograd Block on the same kernels, which takes the same route at functional.FFN_DGRAD_DW3_MIN_ROWS (GPU)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAME, BATCH = "block_base_s0_120x160", 4
KERNEL = "ffn_dgrad_dw3_kernel"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def test_capi_block_takes_the_fused_route_from_65536_rows(monkeypatch):
    import test_block_capi_gpu as capi
    import test_block_gpu as tb
    from dformer_amd import _lib, functional as Fn, kernels as Kk
    from goldens import rel_err
    make = tb.make_block

    def make_batched(name, device="cpu"):  # the golden's Block and weights, BATCH images of its plane
        g, blk, (B, H, W, C, stage, last, dp) = make(name, device)
        return g, blk, (BATCH, H, W, C, stage, last, dp)
    monkeypatch.setattr(tb, "make_block", make_batched)
    _, blk0, (B, H, W, C, stage, last, dp) = make_batched(NAME)
    R = blk0.mlp.fc1.weight.shape[0]
    assert B * H * W >= 65536 == Fn.FFN_DGRAD_DW3_MIN_ROWS
    for c in (C, C // 2):  # RGB and depth ConvFFN
        assert Kk.ffn_dgrad_dw3_supported(torch.bfloat16, (B, H, W), c, R * c // C)
    # the Block's planned workspace covers the kernel's partials
    d = _lib.BlockDesc(B, H, W, C, blk0.attn.num_head, blk0.attn.window, R, int(last), 0, 1e-6)
    assert _lib.lib.dfm_ffn_dgrad_dw3_workspace(B, H, W, R) <= _lib.lib.dfm_block_workspace_size(_lib.BF16, d)

    funcs = (ctypes.c_void_p * 8192)()
    Kk.trace(1)
    try:
        g, last, y, ye, dx, dxe, grads = capi.run_capi(NAME, torch.bfloat16, stack_qcl=True, fused_ffn=0)
        n = _lib.lib.dfm_trace_take(funcs, 8192)
    finally:
        Kk.trace(0)
    names = [Kk.kernel_name(funcs[i]) for i in range(min(n, 8192))]
    assert sum(KERNEL in nm for nm in names) == 2, sorted(set(names))  # RGB and depth ConvFFN backward
    assert not any("dw3_rows_bwd_kernel" in nm or "dw3_stream_bwd_kernel" in nm for nm in names)
    for nm, t in grads.items():
        assert torch.isfinite(t).all(), nm

    Kk.ACCOUNT = []
    Kk.trace(1)
    try:
        _, blk, x_ref, xe_ref, y_ref, ye_ref, _ = tb.run_block(NAME, torch.bfloat16)
    finally:
        Kk.trace(0)
        acct, Kk.ACCOUNT = Kk.ACCOUNT, None
    assert sum(KERNEL in Kk.kernel_name(f) for a in acct for f in a[0]) == 2
    pairs = [("y", y, y_ref), ("dx", dx, x_ref.grad), ("ye", ye, ye_ref), ("dxe", dxe, xe_ref.grad)]
    pairs += [(nm, grads[nm], p.grad) for nm, p in blk.named_parameters() if p.grad is not None]
    bad = {}
    for nm, a, b in pairs:  # test_block_capi_bf16_vs_autograd_path's gate
        e = rel_err(a.detach().float().cpu(), b.detach().float().cpu())
        if not np.isfinite(e) or e > 2e-2:
            bad[nm] = e
    assert not bad, bad
    # the 3x3 weight / bias gradients come from the same kernel on both sides, fed by dh-independent operands
    # that differ only through the forward's GEMM grouping: far inside the gate
    print({nm: rel_err(grads[nm].float().cpu(), dict(blk.named_parameters())[nm].grad.float().cpu())
           for nm in ("mlp.pos.weight", "mlp.pos.bias", "mlp_e2.pos.weight", "mlp_e2.pos.bias") if nm in grads})
