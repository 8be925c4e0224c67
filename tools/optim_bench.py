"""Time the optimizer tail alone: FusedAdamW's options off against all on, over flat buffers.

    python tools/optim_bench.py [--params 29.8e6] [--accum 2] [--reps 30] [--inner 10] [--out profiles/optim_bench.json]

Two flat groups of --params elements in all (DFormer-Base: 29.8 M, nearly all in the decay group), bf16
shadow on the decay group as in the bf16 step. The pieces are timed with HIP events around --inner
back-to-back launches, alternated in one process, median of --reps regions:

  adamw_plain      the tail with the options off (one launch per group, every call)
  accumulate       acc += g (every call with accum_steps > 1)
  norm             sum of squares, both stages (the window's last call)
  adamw_options    the update with clip coefficient, EMA and the accumulator's clear (the window's last call)
  skipped          norm + adamw_options launched inside a window: they return at once (every other call)

Each piece's algorithmic bytes (what kernels.py accounts) over its time is the achieved bytes/s; the
share of HBM rate is against the 6.3 TB/s a float4 copy reaches on the MI355X (8.0 TB/s on paper).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dformer_amd import kernels as K  # noqa: E402

DEV = torch.device("cuda", 0)
HBM_COPY_TBPS = 6.3
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.01


class Group:
    def __init__(self, n, shadow):
        self.p = torch.randn(n, device=DEV)
        self.g = torch.randn(n, device=DEV) * 1e-3
        self.acc = torch.zeros(n, device=DEV)
        self.m = torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV)
        self.ema = self.p.clone()
        self.copy = torch.empty(n, device=DEV, dtype=torch.bfloat16) if shadow else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=float, default=29.8e6)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(a.params)
    small = max(1, n // 200)  # the no-decay group: biases and norm parameters
    groups = [Group(n - small, True), Group(small, False)]
    hyper = torch.tensor([6e-5, 1.0], device=DEV)
    nb = K.sumsq_blocks()
    part = torch.zeros(2 * nb, device=DEV)
    clip = torch.zeros(2, device=DEV)
    last = torch.tensor([a.accum - 1, a.accum], device=DEV, dtype=torch.int32)
    inside = torch.tensor([0, a.accum], device=DEV, dtype=torch.int32)
    gscale = 1.0 / a.accum

    def adamw_plain():
        for g in groups:
            K.adamw(g.p, g.g, g.m, g.v, 0.0, B1, B2, EPS, WD, 1, 1.0, g.copy, hyper=hyper)

    def accumulate():
        for g in groups:
            K.grad_accumulate(g.acc, g.g)

    def norm(win=last):
        for j, g in enumerate(groups):
            K.grad_sumsq(g.acc, part[j * nb:(j + 1) * nb], win=win)
        K.grad_clip_coef(part, gscale, 1.0, clip, win=win)

    def adamw_options(win=last):
        for g in groups:
            K.adamw(g.p, g.acc, g.m, g.v, 0.0, B1, B2, EPS, WD, 1, gscale, g.copy, hyper=hyper, clip_state=clip,
                    win=win, ema=g.ema, ema_decay=0.999, clear_g=True)

    def skipped():
        norm(inside)
        adamw_options(inside)

    shadow = 2 * groups[0].p.numel()
    pieces = {"adamw_plain": (adamw_plain, 28 * n + shadow), "accumulate": (accumulate, 12 * n), "norm": (norm, 4 * n),
              "adamw_options": (adamw_options, 40 * n + shadow), "skipped": (skipped, 0)}
    times = {k: [] for k in pieces}
    for it in range(a.reps + 3):
        for name, (fn, _) in pieces.items():  # alternated: every piece sees the same neighbours and clocks
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                times[name].append(e0.elapsed_time(e1) / a.inner)
    res = {"device": torch.cuda.get_device_name(0), "params": n, "accum_steps": a.accum, "reps": a.reps,
           "launches_per_timed_region": a.inner, "pieces": {}}
    med = {}
    for name, (_, nbytes) in pieces.items():
        med[name] = statistics.median(times[name])
        row = {"median_ms": round(med[name], 4), "min_ms": round(min(times[name]), 4),
               "algorithmic_GB": round(nbytes / 1e9, 3)}
        if nbytes:
            row["achieved_TBps"] = round(nbytes / med[name] / 1e9, 3)
            row["share_of_hbm_copy_rate"] = round(nbytes / med[name] / 1e9 / HBM_COPY_TBPS, 3)
        res["pieces"][name] = row
    k = a.accum
    off = k * med["adamw_plain"]
    on = k * med["accumulate"] + (k - 1) * med["skipped"] + med["norm"] + med["adamw_options"]
    res["window_tail_ms"] = {"options_off": round(off, 4), "all_on": round(on, 4), "extra": round(on - off, 4)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
