"""Time the focal + Tversky criterion, forward + backward, on one MI355X.

    python tools/segterms_bench.py [--iters 300] [--warmup 20] [--out profiles/segterms_bench.json]

Two cases, bf16 low-res logits of a decode head at B = 16, 60 x 80 -> 480 x 640: 40 classes (NYUDepthv2) and 2
classes (the Trav head). Three routes, alternated iteration by iteration in one process, each forward + backward
timed with device events around it (median, 5th / 95th percentile over --iters iterations after --warmup):

  fused   criterion.SegTermsFn: focal_gamma = 2 and region = "tversky" in one pass over the low-res logits
  torch   what a user had before: F.interpolate of the low-res logits to fp32 full resolution, then
          losses.FusedSegLoss.forward (the torch definition) and autograd
  ce      the existing fused cross-entropy for scale: K.seg_loss_fwd_grad + K.seg_loss_bwd_gather

and torch.cuda.max_memory_allocated above the resident inputs for `fused` and `torch`, taken in a run of their
own after the timing. The losses of `fused` and `torch` are printed next to each other.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dformer_amd import kernels as K  # noqa: E402
from dformer_amd.criterion import SegTermsFn  # noqa: E402
from dformer_amd.losses import FusedSegLoss  # noqa: E402

DEV = torch.device("cuda", 0)
B, HL, WL, H, W = 16, 60, 80, 480, 640
GAMMA, REGION = 2.0, (0.3, 0.7, 1.0)


def tensors(ncls):
    g = torch.Generator(device=DEV).manual_seed(ncls)
    rows = (3 * torch.randn(B * HL * WL, ncls, device=DEV, generator=g)).to(torch.bfloat16).requires_grad_()
    lab = torch.randint(0, ncls, (B, H, W), device=DEV, generator=g)
    lab[torch.rand(B, H, W, device=DEV, generator=g) < 0.1] = 255
    weight = 0.5 + 1.5 * torch.rand(ncls, device=DEV, generator=g)
    return rows, lab, weight


def routes(ncls):
    rows, lab, weight = tensors(ncls)
    crit = FusedSegLoss(255, weight, focal_gamma=GAMMA, region="tversky").to(DEV)
    gs = torch.ones(1, device=DEV)

    def fused():
        loss = SegTermsFn.apply(rows, B, HL, WL, lab, 255, weight, GAMMA, True, REGION, 1.0)
        torch.autograd.grad(loss, rows)
        return loss

    def torch_route():
        low = rows.view(B, HL, WL, ncls).permute(0, 3, 1, 2).float()
        loss = crit(F.interpolate(low, (H, W), mode="bilinear", align_corners=False), lab)
        torch.autograd.grad(loss, rows)
        return loss

    def ce():
        out, part = K.seg_loss_fwd_grad(rows.detach(), B, HL, WL, ncls, lab)
        K.seg_loss_bwd_gather(part, B, HL, WL, ncls, out, gs, torch.bfloat16)
        return out[0] / out[1]

    return {"fused": fused, "torch": torch_route, "ce": ce}


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def run_case(ncls, iters, warmup):
    fns = routes(ncls)
    times, loss = {k: [] for k in fns}, {}
    for it in range(warmup + iters):
        for name, fn in fns.items():  # alternate the routes inside one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
            loss[name] = out.item()
    res = {}
    for name, v in times.items():
        res[name] = {"median_ms": round(statistics.median(v), 4), "p05_ms": round(pct(v, 0.05), 4),
                     "p95_ms": round(pct(v, 0.95), 4), "loss": loss[name]}
    for name in ("fused", "torch"):  # peak memory above what is resident before the call
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fns[name]()
        torch.cuda.synchronize()
        res[name]["peak_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    res["torch_over_fused"] = round(res["torch"]["median_ms"] / res["fused"]["median_ms"], 2)
    # the fused route is faster beyond the spread if its slow tail is under the torch route's fast tail
    res["fused_p95_below_torch_p05"] = res["fused"]["p95_ms"] < res["torch"]["p05_ms"]
    res["full_resolution_logits_MiB"] = round(B * ncls * H * W * 4 / 2 ** 20, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segterms_bench: needs a GPU (timings on a CPU say nothing about it)")
    res = {"device": torch.cuda.get_device_name(0), "shape": dict(B=B, low=[HL, WL], label=[H, W], dtype="bfloat16"),
           "criterion": dict(focal_gamma=GAMMA, region="tversky", alpha=REGION[0], beta=REGION[1], smooth=REGION[2]),
           "iters": a.iters, "warmup": a.warmup}
    for ncls in (40, 2):
        res[f"classes_{ncls}"] = run_case(ncls, a.iters, a.warmup)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
