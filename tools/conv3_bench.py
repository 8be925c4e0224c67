"""Time the implicit-GEMM 3x3 conv (csrc/conv3_igemm.hip) against the materialised path of the aux head.

    python tools/conv3_bench.py [--reps 20] [--inner 5] [--dtype bf16] [--out profiles/conv3_bench.json]

Per shape (B, H, W, Cin -> Cout), alternated in one process, HIP-event time of --inner back-to-back calls per
region, median over --reps regions after 3 warm-up regions:
  implicit      forward  = K.conv3_igemm
                backward = K.conv3_igemm_wgrad (+ bias column) + K.conv3_igemm on dy with the flipped pack
  materialised  forward  = K.conv3s1_im2col + K.linear (what Conv3BNReLUFn runs)
                backward = K.linear_wgrad (+ bias column) + K.linear_dgrad + K.conv3s1_col2im, on the saved cols
The weight packs are made once outside the timed regions on both sides (both paths cache or re-pack alike).
Default shapes: the FPN conv of DFormer-Base + UPernet at 480 x 640, bs 16 (16, 120, 160, 512 -> 512: `cols` is
2.8 GB and still fits) and the aux head's conv (16, 30, 40, 256 -> 256). Also prints each side's algorithmic
FLOP/s and the bytes the materialised operand adds. Outputs of the two paths are compared before timing.
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
# fpn8: the FPN conv at bs 8, where `cols` (1.4 GB) stays under the 2 GiB buffer-descriptor limit of dfm_gemm's
# fast loads (at bs 16 the materialised GEMMs take their guarded path: that is what the parent would run there)
SHAPES = {"fpn": (16, 120, 160, 512, 512), "fpn8": (8, 120, 160, 512, 512), "aux": (16, 30, 40, 256, 256)}


def _region(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_shape(shape, dt, reps, inner):
    B, H, W, cin, cout = shape
    P = B * H * W
    torch.manual_seed(0)
    x = torch.randn(P, cin, device=DEV).to(dt)
    dy = torch.randn(P, cout, device=DEV).to(dt)
    w = torch.randn(cout, cin, 3, 3, device=DEV) / (3.0 * cin ** 0.5)
    b = torch.randn(cout, device=DEV)
    wp = K.conv3_weight_pack(w, dt, 9 * cin)
    wpt = K.conv3_weight_pack_dgrad(w, dt)
    cols = K.conv3s1_im2col(x, (B, H, W))
    y, y_old = torch.empty(P, cout, device=DEV, dtype=dt), torch.empty(P, cout, device=DEV, dtype=dt)
    dx, dcols = torch.empty(P, cin, device=DEV, dtype=dt), torch.empty(P, 9 * cin, device=DEV, dtype=dt)

    def imp_fwd():
        K.conv3_igemm(x, (B, H, W), wp, b, out=y)

    def imp_bwd():
        K.conv3_igemm_wgrad(dy, x, (B, H, W), bias_grad=True)
        K.conv3_igemm(dy, (B, H, W), wpt, out=dx)

    def mat_fwd():
        K.conv3s1_im2col(x, (B, H, W), out=cols)
        K.linear(cols, wp, b, out=y_old)

    def mat_bwd():
        K.linear_wgrad(dy, cols, bias_grad=True)
        K.linear_dgrad(dy, wp, out=dcols)
        K.conv3s1_col2im(dcols, (B, H, W), cin, dx=dx)

    # same results first (faster and different is not faster)
    imp_fwd()
    mat_fwd()
    rel = lambda a, c: ((a.float() - c.float()).abs().max() / c.float().abs().max()).item()  # noqa: E731
    agree = {"y": rel(y, y_old)}
    dwp_i, db_i = K.conv3_igemm_wgrad(dy, x, (B, H, W), bias_grad=True)
    dwp_m, db_m = K.linear_wgrad(dy, cols, bias_grad=True)
    agree["dwp"], agree["db"] = rel(dwp_i, dwp_m), rel(db_i, db_m)
    imp_dx = K.conv3_igemm(dy, (B, H, W), wpt).clone()
    mat_bwd()
    agree["dx"] = rel(imp_dx, dx)
    del dwp_i, dwp_m, imp_dx
    runs = {"implicit_fwd": imp_fwd, "materialised_fwd": mat_fwd, "implicit_bwd": imp_bwd, "materialised_bwd": mat_bwd}
    times = {k: [] for k in runs}
    for it in range(reps + 3):
        for name, fn in runs.items():  # alternate the two paths inside one process
            t = _region(fn, inner)
            if it >= 3:
                times[name].append(t)
    es = x.element_size()
    flop = 2.0 * P * cout * 9 * cin
    out = {"shape": list(shape), "dtype": str(dt), "agreement_rel_to_max": {k: float(f"{v:.3e}") for k, v in agree.items()},
           "cols_GB": round(P * 9 * cin * es / 1e9, 3), "fwd_GFLOP": round(flop / 1e9, 1)}
    for k, v in times.items():
        med = statistics.median(v)
        nfl = flop * (2 if k.endswith("bwd") else 1)
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "TFLOPs": round(nfl / med / 1e9, 1)}
    for leg in ("fwd", "bwd"):
        out[f"implicit_over_materialised_{leg}"] = round(out[f"implicit_{leg}"]["median_ms"] /
                                                         out[f"materialised_{leg}"]["median_ms"], 4)
    tot_i = out["implicit_fwd"]["median_ms"] + out["implicit_bwd"]["median_ms"]
    tot_m = out["materialised_fwd"]["median_ms"] + out["materialised_bwd"]["median_ms"]
    out["fwd_plus_bwd_ms"] = {"implicit": round(tot_i, 4), "materialised": round(tot_m, 4),
                              "implicit_over_materialised": round(tot_i / tot_m, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls per timed region")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--shapes", default="fpn,fpn8,aux", help="comma list of " + ", ".join(SHAPES) + " or B,H,W,Cin,Cout")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    names = a.shapes.split(",")
    shapes = [tuple(int(v) for v in names)] if len(names) == 5 and names[0].isdigit() else [SHAPES[n] for n in names]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "calls_per_region": a.inner,
           "shapes": [bench_shape(s, dt, a.reps, a.inner) for s in shapes]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
