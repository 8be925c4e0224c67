"""Time sliding-window multi-scale evaluation on the GPU: the fused kernel against the torch composition.

    python tools/slide_eval_time.py [--out FILE] [--reps N] [--dtypes fp32 bf16]

DFormer-Base + ham on one seeded synthetic batch of 2 images at 530x730 (the SUN-RGBD evaluation
shape), crop 480x480, stride rate 2/3, scales 0.5 ... 1.5 with flip. Per dtype, in a child process of
its own under a time limit (a failed step ends the run), after warm-up, alternating the variants and
timing each repetition with device events:
  (a)  evaluate_msf(..., sliding=True): one dfm_slide_msf_accumulate launch per scale and flip
  (b)  the same loop with everything after the model done the reference's way in torch: upsample each
       window's logits, zero-pad to the scaled size, sum, count map, divide, flip, resize, softmax, add
  post-model alone: both forms of that tail on the same pre-computed window logits
and the kernel's own time per launch next to its bytes from shapes (the read-modify-write of the score
buffer, B*H*W*ncls*8, plus one read of every window's low-res logits). Reads nothing outside the tree.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)
B, H, W, NCLS, CROP, RATE = 2, 530, 730, 37, (480, 480), 2 / 3


class Cfg(dict):
    __getattr__ = dict.__getitem__


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(v):
    return f"median {statistics.median(v):9.3f} ms  (min {min(v):9.3f}, max {max(v):9.3f}, n={len(v)})"


def worker(dtype, reps, crop_batch):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from dformer_amd import kernels as K
    from dformer_amd import evaluate as E
    from dformer_amd.segmentor import EncoderDecoder
    if not torch.cuda.is_available():
        raise SystemExit("slide_eval_time: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(8964)
    cfg = Cfg(backbone="DFormer-Base", decoder="ham", decoder_embed_dim=512, num_classes=NCLS, drop_path_rate=0.1,
              bn_eps=1e-3, bn_momentum=0.1, background=255, eval_crop_size=list(CROP), eval_stride_rate=RATE)
    if crop_batch:
        cfg["eval_crop_batch"] = crop_batch
    model = EncoderDecoder(cfg=cfg).to(dev).eval()
    if dtype == "bf16":
        model.set_compute_dtype(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(8964)
    rgb = torch.randn(B, 3, H, W, device=dev, generator=g)
    dep = torch.randn(B, 1, H, W, device=dev, generator=g)
    gt = torch.randint(0, NCLS, (B, H, W), device=dev, generator=g)
    loader = [{"rgb": rgb, "modal_x": dep, "gt": gt}]
    slide = E._slide_config(cfg)  # crop, strides and cfg's crops per model call
    strides = slide.strides
    combos = [(s, f) for s in SCALES for f in (False, True)]

    def inputs(scale, flip):
        size = E.msf_size(H, W, scale)
        return K.resize_nchw(rgb, size, True, flip=flip), K.resize_nchw(dep, size, True, flip=flip)

    def torch_tail(rows, b, h, w, scaled, flip, scores):
        """val_mm.py:297-319 + 377-397 on the windows' low-res logits."""
        Hs, Ws = scaled
        wins = [(y1, y2, x1, x2) for y1, y2 in E.slide_windows(Hs, CROP[0], strides[0])
                for x1, x2 in E.slide_windows(Ws, CROP[1], strides[1])]
        low = rows.view(len(wins), b, h, w, NCLS).permute(0, 1, 4, 2, 3)
        preds = torch.zeros(b, NCLS, Hs, Ws, device=dev)
        count = torch.zeros(b, 1, Hs, Ws, device=dev)
        for i, (y1, y2, x1, x2) in enumerate(wins):
            up = F.interpolate(low[i].float(), size=CROP, mode="bilinear", align_corners=False)
            preds += F.pad(up, (x1, Ws - x2, y1, Hs - y2))
            count[:, :, y1:y2, x1:x2] += 1
        logits = preds / count
        if flip:
            logits = torch.flip(logits, dims=(3,))
        scores += F.interpolate(logits, size=(H, W), mode="bilinear", align_corners=True).softmax(dim=1)

    @torch.no_grad()
    def variant_a():
        return E.evaluate_msf(model, loader, cfg, dev, list(SCALES), True, sliding=True)

    @torch.no_grad()
    def variant_b():
        metrics = E.Metrics(NCLS, 255, dev)
        scores = torch.zeros(B, NCLS, H, W, device=dev)
        for scale, flip in combos:
            x, e = inputs(scale, flip)
            rows, (b, h, w), scaled = E._slide_low_rows(model, x, e, slide)
            torch_tail(rows, b, h, w, scaled, flip, scores)
        metrics.update(scores, gt)
        return metrics

    with torch.no_grad():
        lows = []
        for scale, flip in combos:
            x, e = inputs(scale, flip)
            lows.append(E._slide_low_rows(model, x, e, slide) + (flip,))
    acc = torch.zeros(B * H * W, NCLS, device=dev)
    scores = torch.zeros(B, NCLS, H, W, device=dev)

    def post_fused():
        for rows, (b, h, w), scaled, flip in lows:
            K.slide_msf_accumulate(rows, b, h, w, NCLS, CROP, strides, scaled, (H, W), flip, acc)

    def post_torch():
        for rows, (b, h, w), scaled, flip in lows:
            torch_tail(rows, b, h, w, scaled, flip, scores)

    ma, mb = variant_a(), variant_b()  # warm-up, and the two variants must agree
    post_fused()
    post_torch()
    torch.cuda.synchronize()
    flips = (ma.hist - mb.hist).abs().sum().item() / 2
    ta, tb, pf, pt = [], [], [], []
    for _ in range(reps):
        ta.append(timed(variant_a))
        tb.append(timed(variant_b))
        pf.append(timed(post_fused))
        pt.append(timed(post_torch))
    print(f"== DFormer-Base + ham, {dtype}, {B} x {H}x{W}, {NCLS} classes, crop {CROP}, stride {strides}, scales "
          f"{SCALES} + flip, {crop_batch or B} crops per model call; low-res logits {lows[0][0].dtype}")
    print(f"(a) evaluate_msf(sliding=True), fused kernel : {spread(ta)}")
    print(f"(b) same loop, torch composition after model : {spread(tb)}")
    print(f"post-model alone, fused (10 launches)        : {spread(pf)}")
    print(f"post-model alone, torch composition          : {spread(pt)}")
    print(f"argmax differences (a) vs (b): {flips:.0f} of {B * H * W} pixels")
    print("dfm_slide_msf_accumulate per launch (not flipped / flipped alternate inside each scale):")
    for (scale, flip), (rows, (b, h, w), scaled, _) in zip(combos, lows):
        if flip:
            continue
        G = rows.shape[0] // (b * h * w)
        nbytes = B * H * W * NCLS * 8 + rows.numel() * rows.element_size()
        t = [timed(lambda: K.slide_msf_accumulate(rows, b, h, w, NCLS, CROP, strides, scaled, (H, W), False, acc))
             for _ in range(max(reps, 5))]
        med = statistics.median(t)
        print(f"  scale {scale:4.2f}: scaled {scaled[0]}x{scaled[1]}, {G} windows of {h}x{w} logits, "
              f"{nbytes / 1e6:7.2f} MB from shapes, {med * 1e3:8.1f} us (min {min(t) * 1e3:.1f}), "
              f"{nbytes / med / 1e6:7.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report here")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--crop-batch", type=int, default=0, help="crops per model call (default: one window of the batch)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds per dtype step")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        worker(args.step, args.reps, args.crop_batch)
        return 0
    report = []
    for dt in args.dtypes:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", dt, "--reps", str(args.reps), "--crop-batch",
               str(args.crop_batch)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"slide_eval_time: {dt} step exceeded {args.step_timeout:.0f} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"slide_eval_time: {dt} step failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        report.append(r.stdout)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
