"""Time the DFormerTrav laser-scan expansion: the two kernels alone, and what the backbone adds to a step.

    python tools/laser_bench.py [--batch 16] [--reps 30] [--steps 20] [--out profiles/laser_bench.json]

1. The kernels of dfm_laser_expand_fwd / _bwd at [batch] scans of 360 ranges -> 480 x 640 planes, timed by the
   library's launch tracer (HIP events around each launch), median of --reps launches, with the achieved
   bytes/s against their algorithmic bytes (kernels.laser_expand_fwd / _bwd's accounting: scan, alpha, g, c in;
   s, moments and the plane out / the plane's gradient and the moments in; ds, dalpha, dg, dc out).
2. The training step of DFormerTrav-Base + ham (bf16, FusedAdamW, HIP-graph replay) on a scan, alternated in one
   process with plain DFormer-Base + ham on a synthetic depth image of the same batch: HIP-event time of
   --steps replays per region, median over --reps regions. The difference is the whole cost of the expansion:
   the fold, the two laser entry points and the first depth-stem conv's now-live Cin = 1 input gradient (dgrad
   GEMM + col2im), which plain DFormer skips because a depth image needs no gradient.
3. Those parts one by one, each replayed from a HIP graph of its own: the fold with its backward, the whole
   expansion module forward + backward, the first depth-stem conv with and without its input gradient.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from dformer_amd import kernels as K  # noqa: E402
from dformer_amd.segmentor import EncoderDecoder  # noqa: E402
from dformer_amd.train import FusedAdamW, GraphedTrainStep  # noqa: E402

DEV = torch.device("cuda", 0)
N, L, HOUT, HH = 360, 640, 480, 4


def kernel_times(B, reps):
    torch.manual_seed(0)
    x = torch.rand(B, N, device=DEV) * 9.5 + 0.5
    alpha = torch.randn(L, HH, device=DEV)
    g = torch.rand(HH, device=DEV) + 0.3
    c = torch.zeros(1, device=DEV)
    dplane = torch.randn(B, HOUT, L, device=DEV)
    plane, s, mean, var = K.laser_expand_fwd(x, alpha, g, c, HOUT)
    byt = {"laser_expand_fwd_kernel (train: with moments)": 4 * (B * N + L * HH + HH + 1 + B * L + B * HOUT * L
                                                                  + 2 * B * L * HH),
           "laser_expand_fwd_kernel (eval: no moments)": 4 * (B * N + L * HH + HH + 1 + B * L + B * HOUT * L),
           "laser_rowsum_kernel": 4 * (B * HOUT * L + B * L),
           "laser_param_grad_kernel": 4 * (B * L + 2 * B * L * HH + L * HH + HH),
           "laser_param_grad_final_kernel": 4 * (HH + 1)}
    runs = {"laser_expand_fwd_kernel (train: with moments)": lambda: K.laser_expand_fwd(x, alpha, g, c, HOUT),
            "laser_expand_fwd_kernel (eval: no moments)": lambda: K.laser_expand_fwd(x, alpha, g, c, HOUT, save=False),
            "laser_rowsum_kernel": lambda: K.laser_expand_bwd(dplane, g, mean, var),
            "laser_param_grad_kernel": lambda: K.laser_expand_bwd(dplane, g, mean, var),
            "laser_param_grad_final_kernel": lambda: K.laser_expand_bwd(dplane, g, mean, var)}
    out = {}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        K.trace(2)
        for _ in range(reps):
            fn()
        ts = [ms * 1e3 for nm, ms in K.trace_read() if name.split(" ")[0] in nm]
        K.trace(0)
        assert len(ts) == reps, (name, len(ts))
        med = statistics.median(ts)
        out[name] = {"median_us": round(med, 1), "min_us": round(min(ts), 1), "algorithmic_MB": round(byt[name] / 1e6, 2),
                     "achieved_GBps": round(byt[name] / med / 1e3, 1)}
    return out


def _replay_ms(fn, reps, inner=20):
    """Median HIP-event time per replay of fn captured into a HIP graph (what a graphed step pays for it)."""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    ts = []
    for it in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            graph.replay()
        e1.record()
        e1.synchronize()
        if it >= 3:
            ts.append(e0.elapsed_time(e1) / inner)
    return round(statistics.median(ts), 4)


def part_times(B, reps):
    """Where the backbone's extra time goes, each part replayed from its own HIP graph: the parameter fold
    with its autograd backward (small float64 tensor ops), the whole expansion module forward + backward, and
    the first depth-stem conv (Cin = 1 -> 16, bf16) with and without its input gradient."""
    from dformer_amd.encoder import Attention1Dto2D, ConvS2Fn
    torch.manual_seed(0)
    mod = Attention1Dto2D(N, L, HOUT, 64, HH).to(DEV)
    scan = torch.rand(B, 1, N, device=DEV) * 9.5 + 0.5
    gy = torch.randn(B, 1, HOUT, L, device=DEV)

    def fold():
        a, g, c = mod.fold()
        torch.autograd.grad(a.sum() + g.sum() + c.sum(), list(mod.parameters()), allow_unused=True)

    def module():
        torch.autograd.grad(mod(scan), list(mod.parameters()), gy, allow_unused=True)

    conv = torch.nn.Conv2d(1, 16, 3, 2, 1).to(DEV)
    plane = torch.randn(B, 1, HOUT, L, device=DEV)
    leaf = plane.clone().requires_grad_()
    dy = torch.randn(B * (HOUT // 2) * (L // 2), 16, device=DEV).to(torch.bfloat16)

    def stem(x, wrt):
        y = ConvS2Fn.apply(x, conv.weight, conv.bias, None, None, None, False, False, torch.bfloat16)
        torch.autograd.grad(y, wrt, dy)

    out = {"fold_fwd_bwd_ms": _replay_ms(fold, reps), "expansion_module_fwd_bwd_ms": _replay_ms(module, reps),
           "stem_conv1_fwd_bwd_ms": _replay_ms(lambda: stem(plane, [conv.weight, conv.bias]), reps),
           "stem_conv1_fwd_bwd_with_input_grad_ms": _replay_ms(lambda: stem(leaf, [leaf, conv.weight, conv.bias]), reps)}
    out["stem_conv1_input_grad_ms"] = round(out["stem_conv1_fwd_bwd_with_input_grad_ms"] - out["stem_conv1_fwd_bwd_ms"], 4)
    return out


def graphed(arch, B, H, W):
    cfg = bench.make_cfg(arch, "ham")
    torch.manual_seed(0)
    m = EncoderDecoder(cfg=cfg).to(DEV).set_compute_dtype(torch.bfloat16).train()
    m.return_logits = False
    opt = FusedAdamW(m, lr=cfg.lr, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
    rgb, dep, lab = bench.synthetic_batch(B, H, W, cfg.num_classes, DEV, 0)
    if arch.startswith("DFormerTrav"):
        dep = torch.rand(B, 1, N, device=DEV) * 9.5 + 0.5
    return GraphedTrainStep(m, opt, rgb, dep, lab, warmup=2)


def step_times(B, reps, steps):
    steps_of = {"DFormer-Base": graphed("DFormer-Base", B, HOUT, L), "DFormerTrav-Base": graphed("DFormerTrav-Base", B, HOUT, L)}
    times = {k: [] for k in steps_of}
    for it in range(reps + 3):
        for name, g in steps_of.items():  # alternate the two models inside one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                g()
            e1.record()
            e1.synchronize()
            if it >= 3:
                times[name].append(e0.elapsed_time(e1) / steps)
    out = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
           for k, v in times.items()}
    out["trav_minus_base_ms"] = round(out["DFormerTrav-Base"]["median_ms"] - out["DFormer-Base"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20, help="graph replays per timed region")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "shape": dict(N=N, L=L, Hout=HOUT, Hh=HH),
           "reps": a.reps, "kernels": kernel_times(a.batch, a.reps)}
    if not a.no_step:
        res["parts"] = part_times(a.batch, a.reps)
        res["replays_per_timed_region"] = a.steps
        res["step"] = step_times(a.batch, a.reps, a.steps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
