"""Time the evaluation tail of one batch: low-res logits -> confusion histogram.

    python tools/eval_tail_bench.py [--reps 30] [--inner 20] [--out profiles/eval_tail.json]

Per case (16x480x640 labels; bf16 low-res logits of 60x80 x 40 classes, the ham head, and of 120x160 x 37
classes, the MLP head) it compares, alternating in one process, HIP-event timed, median of --reps regions of
--inner back-to-back calls each (time per call; one call per region would time the host's way to the launch, the
GPU being idle when the first event is recorded):
  fused       Metrics.update_low (K.seg_predict, histogram only)
  fused+pred  the same, also writing the uint8 class map
  upsample    EncoderDecoder._upsample (K.bilinear to [B, ncls, H, W]) + Metrics.update
  msf         K.msf_accumulate (the sliding-window accumulate kernel on one window) into a zeroed
              [B*H*W, ncls] buffer + Metrics.update_rows (the rows_argmax kernel with a label): what
              evaluate_msf(scales=[1], flip=False) does per batch
and reports the dfm_seg_predict kernel alone (the library's launch tracer), the achieved bytes/s against the algorithmic bytes of DESIGN.md §3 (ncls * es per low-res pixel
+ 8 B label [+ 1 B prediction] per output pixel) and the peak memory each path allocates.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dformer_amd import kernels as K  # noqa: E402
from dformer_amd.evaluate import Metrics  # noqa: E402
from dformer_amd.segmentor import EncoderDecoder  # noqa: E402

DEV = "cuda"


def run_case(B, H, W, h, w, ncls, dtype, reps, warmup, inner):
    torch.manual_seed(0)
    rows = torch.randn(B * h * w, ncls, device=DEV).to(dtype)
    low = rows.view(B, h, w, ncls).permute(0, 3, 1, 2)  # the decode head's NCHW view of NHWC rows
    gt = torch.randint(0, ncls, (B, H, W), device=DEV)
    gt[torch.rand(B, H, W, device=DEV) < 0.1] = 255
    pred = torch.empty(B, H, W, device=DEV, dtype=torch.uint8)

    def fused(m):
        m.update_low(rows, (B, h, w), gt)

    def fused_pred(m):
        m.update_low(rows, (B, h, w), gt, pred=pred)

    def upsample(m):
        m.update(EncoderDecoder._upsample(None, low, (H, W)), gt)

    def msf(m):
        acc = torch.zeros(B * H * W, ncls, device=DEV, dtype=torch.float32)
        K.msf_accumulate(rows, B, h, w, ncls, (H, W), (H, W), False, acc)
        m.update_rows(acc, gt)

    paths = {"fused": fused, "fused+pred": fused_pred, "upsample": upsample, "msf": msf}
    hists, times, peak = {}, {k: [] for k in paths}, {}
    for name, fn in paths.items():
        m = Metrics(ncls, 255, DEV)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(m)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        hists[name] = m._hist.clone()
    m = Metrics(ncls, 255, DEV)
    for it in range(warmup + reps):
        for name, fn in paths.items():  # alternate the paths inside one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn(m)
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    # the kernel alone (the library's launch tracer: HIP events around each launch), also without the label
    kern = {}
    for name, fn in (("fused", fused), ("fused+pred", fused_pred),
                     ("pred only", lambda m: K.seg_predict(rows, B, h, w, ncls, (H, W), pred=pred))):
        K.trace(2)
        for _ in range(reps):
            fn(m)
        ts = [ms * 1e3 for nm, ms in K.trace_read() if "seg_predict" in nm]
        K.trace(0)
        assert len(ts) == reps, (name, len(ts))
        kern[name] = round(statistics.median(ts), 1)
    npix = B * H * W
    alg = {"fused": B * h * w * ncls * rows.element_size() + 8 * npix}
    alg["fused+pred"] = alg["fused"] + npix
    out = {"case": dict(B=B, H=H, W=W, h=h, w=w, ncls=ncls, dtype=str(dtype).replace("torch.", "")), "reps": reps,
           "calls_per_timed_region": inner,
           "seg_predict_kernel_us": kern, "paths": {}}
    for name in paths:
        ts = sorted(times[name])
        med = statistics.median(ts)
        r = {"median_us": round(med, 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1),
             "peak_alloc_MB": round(peak[name] / 1e6, 1),
             "hist_moved_vs_fused": int((hists[name] - hists["fused"]).abs().sum().item()) // 2}
        if name in alg:
            r["algorithmic_MB"] = round(alg[name] / 1e6, 2)
            r["achieved_GBps"] = round(alg[name] / med / 1e3, 1)
        out["paths"][name] = r
    f = out["paths"]["fused"]["median_us"]
    out["speedup_vs_upsample"] = round(out["paths"]["upsample"]["median_us"] / f, 1)
    out["speedup_vs_msf"] = round(out["paths"]["msf"]["median_us"] / f, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dformer_amd import _lib
    res = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(_lib.LIB_PATH), "cases": [
        run_case(16, 480, 640, 60, 80, 40, torch.bfloat16, a.reps, a.warmup, a.inner),
        run_case(16, 480, 640, 120, 160, 37, torch.bfloat16, a.reps, a.warmup, a.inner)]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
