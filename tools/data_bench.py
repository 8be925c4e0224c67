"""Time the input-pipeline kernel (dformer_amd.data.TrainPre, libdformer_data.so) against the same pipeline as a
chain of torch ops on the same device, and against its algorithmic bytes.

    python tools/data_bench.py [--batch 16] [--reps 30] [--inner 20] [--out profiles/data_bench.json]

The batch is [batch] raw 480 x 640 images (uint8 rgb, 1-channel modal, label) cropped to 480 x 640 with the
reference's train_scale_array drawn per sample (TrainPre.draw, seed 0): mixed scales, mirrors and crop positions.

* kernel: HIP events around --inner back-to-back launches, median over --reps regions after warm-up. The launches
  rotate over 4 sets of input and output tensors (4 x 143 MB at batch 16), so the 256 MB Infinity Cache cannot
  hold a launch's outputs for the next one; a loader writes buffers the training step has since evicted.
* torch chain: per sample (the scales differ) flip, F.interpolate(bilinear) in fp32, round to the grey-level
  lattice, normalise, index the label, crop, pad and copy into the same output tensors, timed the same way with a
  quarter of the launches per region. Its outputs are compared with the kernel's (share of equal labels, share of
  image pixels on the same grey level): fp32 source coordinates instead of exact integers move a few near ties.
* algorithmic bytes: the outputs (4 float32 planes and one int64 plane per pixel) plus, per sample, the part of the
  raw 1.54 MB that the crop window maps onto (all of it at scales <= 1, about 1/s^2 of it above). Achieved bytes/s =
  those bytes over the kernel time, as a fraction of the 6.3 TB/s float4-copy rate and of the 8 TB/s HBM spec.
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dformer_amd.data import TrainPre  # noqa: E402

DEV = torch.device("cuda", 0)
H0, W0, CH, CW = 480, 640, 480, 640
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MODAL_MEAN, MODAL_STD = [0.48], [0.28]
SCALES = [0.5, 0.75, 1, 1.25, 1.5, 1.75]
SETS = 4


def algorithmic_bytes(rows):
    out = len(rows) * CH * CW * (4 * 4 + 8)
    src = 0.0
    for _, sh, sw, pos_h, pos_w in rows:
        hc, wc = min(sh - pos_h, CH), min(sw - pos_w, CW)
        src += H0 * W0 * 5 * min(1.0, hc * wc / (sh * sw))
    return out, int(src)


def torch_chain(rgb_u8, modal_u8, gt_u8, rows, out):
    mean = torch.tensor(MEAN, device=DEV).view(3, 1, 1)
    std = torch.tensor(STD, device=DEV).view(3, 1, 1)
    for b, (flip, sh, sw, pos_h, pos_w) in enumerate(rows):
        img = torch.cat([rgb_u8[b].permute(2, 0, 1), modal_u8[b][None]]).float()[None]
        g = gt_u8[b]
        if flip:
            img, g = img.flip(-1), g.flip(-1)
        if (sh, sw) != (H0, W0):
            img = torch.floor(F.interpolate(img, size=(sh, sw), mode="bilinear", align_corners=False) + 0.5)
            ys = torch.clamp(torch.arange(sh, device=DEV) * H0 // sh, max=H0 - 1)
            xs = torch.clamp(torch.arange(sw, device=DEV) * W0 // sw, max=W0 - 1)
            g = g[ys][:, xs]
        img = img[0, :, pos_h:pos_h + CH, pos_w:pos_w + CW] / 255.0
        g = g[pos_h:pos_h + CH, pos_w:pos_w + CW].long()
        ph, pw = CH - img.shape[1], CW - img.shape[2]
        margins = (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)
        out[0][b] = F.pad((img[:3] - mean) / std, margins)
        out[1][b] = F.pad((img[3:] - MODAL_MEAN[0]) / MODAL_STD[0], margins)
        out[2][b] = F.pad(g, margins, value=255)


def timed(fn, reps, inner):
    for i in range(2 * SETS):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for it in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(inner):
            fn(it * inner + i)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="kernel launches per timed region")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.batch
    pre = TrainPre(MEAN, STD, (CH, CW), SCALES, MODAL_MEAN, MODAL_STD)
    params = pre.draw(B, (H0, W0), random.Random(0))
    rows = [tuple(r[:5]) for r in params.tolist()]
    dparams = params.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    ins = [(torch.randint(0, 256, (B, H0, W0, 3), device=DEV, dtype=torch.uint8, generator=g),
            torch.randint(0, 256, (B, H0, W0), device=DEV, dtype=torch.uint8, generator=g),
            torch.randint(0, 41, (B, H0, W0), device=DEV, dtype=torch.uint8, generator=g)) for _ in range(SETS)]
    outs = [(torch.empty(B, 3, CH, CW, device=DEV), torch.empty(B, 1, CH, CW, device=DEV),
             torch.empty(B, CH, CW, device=DEV, dtype=torch.int64)) for _ in range(SETS)]

    kern = timed(lambda i: pre(*ins[i % SETS], dparams, out=outs[i % SETS]), a.reps, a.inner)
    got = [t.clone() for t in pre(*ins[0], dparams, out=outs[0])]
    chain = timed(lambda i: torch_chain(*ins[i % SETS], rows, outs[i % SETS]), a.reps, max(1, a.inner // 4))
    torch_chain(*ins[0], rows, outs[0])
    torch.cuda.synchronize()
    same = {"labels_equal": round((got[2] == outs[0][2]).double().mean().item(), 6),
            "rgb_same_grey_level": round(((got[0] - outs[0][0]).abs() < 1e-3).double().mean().item(), 6),
            "modal_same_grey_level": round(((got[1] - outs[0][1]).abs() < 1e-3).double().mean().item(), 6)}

    out_b, src_b = algorithmic_bytes(rows)
    rate = (out_b + src_b) / (kern["median_ms"] * 1e-3)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "raw": [H0, W0], "crop": [CH, CW],
           "scales_drawn": sorted({round(r[1] / H0, 2) for r in rows}), "mirrored": sum(r[0] for r in rows),
           "reps": a.reps, "launches_per_region": a.inner, "buffer_sets": SETS,
           "kernel": kern, "torch_chain": chain,
           "speedup_over_torch_chain": round(chain["median_ms"] / kern["median_ms"], 1),
           "torch_chain_vs_kernel": same,
           "algorithmic_MB": {"outputs": round(out_b / 1e6, 1), "sources": round(src_b / 1e6, 1)},
           "achieved_TBps": round(rate / 1e12, 3), "of_copy_rate_6.3TBps": round(rate / 6.3e12, 3),
           "of_hbm_spec_8TBps": round(rate / 8e12, 3),
           "images_per_s": round(B / (kern["median_ms"] * 1e-3))}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
