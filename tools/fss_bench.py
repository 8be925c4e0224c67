"""Time the few-shot tail of meta_forward at the Trav config's episode: B = 2, S = 5, 480 x 640.

    python tools/fss_bench.py [--reps 30] [--inner 10] [--no-step] [--out profiles/fss_bench.json]

1. Every fss kernel, timed by the library's launch tracer (HIP events around each launch), median of --reps
   launches, with its algorithmic bytes and the achieved bytes/s.
2. The tail, forward + backward, on fixed stage-3 rows [B*S + B, 15, 20, 512] and decode-head logits
   [B, 60, 80, 2] (bf16): the fused tail (FssProtoSimFn + FssLossFn) alternated in one process with the same
   tail composed from the kernels the library had before: K.bilinear of the stage-3 rows to full resolution,
   a masked K.colsum per class, torch ops for the cosine and the softmax, two K.bilinear + torch's cross-entropy,
   and K.bilinear_bwd for every upsample in the backward. HIP-event time of --inner runs per region, median over
   --reps regions, and the peak allocated memory of each. The encoder and the decode head are the same in both,
   so the difference of the tails is the difference of the episode steps.
3. The eager episode step itself (meta_train_step, DFormerTrav-Base + ham, bf16, FusedAdamW): time and peak memory.
"""
import argparse
import json
import os
import re
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from dformer_amd import kernels as K  # noqa: E402
from dformer_amd.decoders import FssLossFn, FssProtoSimFn  # noqa: E402

DEV = torch.device("cuda", 0)
B, S, H, W, HS, WS, HL, WL, C = 2, 5, 480, 640, 15, 20, 60, 80, 512
ALPHA, T = 0.5, 1.0


def episode_tensors(dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(0)
    n = B * S + B
    f3 = torch.randn(n, HS, WS, C, device=DEV, generator=g).to(dtype).permute(0, 3, 1, 2)  # NCHW view of NHWC rows
    low = torch.randn(B * HL * WL, 2, device=DEV, generator=g).to(dtype)
    mask = torch.zeros(B * S, H, W, dtype=torch.int64, device=DEV)
    for i in range(B * S):
        mask[i, 40 * i:40 * i + 200, 50 * i:50 * i + 260] = 1
        mask[i, 300:304] = 255
    lab = mask[:B].clone()
    return f3, low, mask, lab


def kernel_times(reps):
    f3, low, mask, lab = episode_tensors()
    rows = f3.permute(0, 2, 3, 1).reshape(-1, C)
    cells, ns = HS * WS, B * S * HS * WS
    sup, qry = rows[:ns], rows[ns:]
    foot, count = K.fss_mask_footprint(mask, (HS, WS))
    proto, wgt = K.fss_proto_pool_fwd(sup, foot, count, B, S)
    prob, saved = K.fss_sim_fwd(qry, proto, T)
    out, gplane = K.fss_loss_fwd(low, B, HL, WL, prob, HS, WS, lab, ALPHA)
    dprob = torch.randn_like(prob)
    dproto = torch.randn_like(proto)
    calls = {"mask_footprint": lambda: K.fss_mask_footprint(mask, (HS, WS)),
             "proto_pool_fwd": lambda: K.fss_proto_pool_fwd(sup, foot, count, B, S),
             "proto_pool_bwd": lambda: K.fss_proto_pool_bwd(wgt, dproto, B, S, rows.dtype),
             "sim_fwd": lambda: K.fss_sim_fwd(qry, proto, T),
             "sim_bwd": lambda: K.fss_sim_bwd(qry, proto, dprob, prob, saved, T),
             "loss_fwd": lambda: K.fss_loss_fwd(low, B, HL, WL, prob, HS, WS, lab, ALPHA),
             "loss_bwd": lambda: K.fss_loss_bwd(gplane, B, HL, WL, HS, WS, out, ALPHA, low.dtype),
             "fuse_fwd": lambda: K.fss_fuse(low, B, HL, WL, prob, HS, WS, (H, W), ALPHA)}
    res = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        K.ACCOUNT = []
        K.trace(1)
        fn()
        K.trace(0)
        (funcs, _, nbytes, _, _), K.ACCOUNT = K.ACCOUNT[0], None
        K.trace(2)
        for _ in range(reps):
            fn()
        ts = {}
        for nm, ms in K.trace_read():
            ts.setdefault(re.search(r"\w+_kernel", nm).group(0), []).append(ms * 1e3)
        K.trace(0)
        per = {k: round(statistics.median(v) * (len(v) // reps), 2) for k, v in ts.items()}  # a kernel launched twice counts twice
        total = sum(per.values())
        res[name] = {"kernels_median_us": per, "total_us": round(total, 2), "launches": len(funcs),
                     "algorithmic_MB": round(nbytes / 1e6, 3), "achieved_TBps": round(nbytes / total / 1e6, 3)}
    return res


class BilinearFn(torch.autograd.Function):
    """K.bilinear with K.bilinear_bwd as its backward: [B*h*w, C] rows -> [B*H*W, C] rows."""

    @staticmethod
    def forward(ctx, x, in_hw, out_hw, n):
        ctx.meta = (in_hw, out_hw, n)
        return K.bilinear(x.contiguous(), in_hw, out_hw, n)

    @staticmethod
    def backward(ctx, dy):
        in_hw, out_hw, n = ctx.meta
        return K.bilinear_bwd(dy.contiguous(), in_hw, out_hw, n), None, None, None


class MaskedColsumFn(torch.autograd.Function):
    """sum_rows m[r] * x[r, :] by K.colsum(rowscale=m); backward m x dy."""

    @staticmethod
    def forward(ctx, x, m):
        ctx.save_for_backward(m)
        ctx.dtype = x.dtype
        return K.colsum(x, rowscale=m)

    @staticmethod
    def backward(ctx, dy):
        (m,) = ctx.saved_tensors
        return (m[:, None] * dy[None, :]).to(ctx.dtype), None


def composed_tail(f3, low, mask, lab):
    """The tail as the reference states it, on the kernels the library had: every upsample materialised."""
    rows = f3.permute(0, 2, 3, 1).reshape(-1, C)
    cells = HS * WS
    protos = []
    for i in range(B * S):  # per support image, as builder.py:277-284
        up = BilinearFn.apply(rows[i * cells:(i + 1) * cells], (HS, WS), (H, W), 1)
        per = []
        for k in (0, 1):
            m = (mask[i] == k).reshape(-1).float()
            per.append(MaskedColsumFn.apply(up, m) / (m.sum() + 1e-5))
        protos.append(torch.stack(per))
    proto = torch.stack(protos).view(B, S, 2, C).mean(1)
    q = rows[B * S * cells:].view(B, cells, C).float()
    cos = F.cosine_similarity(q[:, :, None, :], proto[:, None, :, :], dim=-1)
    prob = torch.softmax(20.0 * cos / T, -1).reshape(-1, 2)
    fused = ALPHA * BilinearFn.apply(low.float(), (HL, WL), (H, W), B) + \
        (1.0 - ALPHA) * BilinearFn.apply(prob, (HS, WS), (H, W), B)
    keep = lab.reshape(-1) != 255
    return F.cross_entropy(fused[keep], lab.reshape(-1)[keep])


def fused_tail(f3, low, mask, lab):
    foot, count = K.fss_mask_footprint(mask, (HS, WS))
    _, prob, _ = FssProtoSimFn.apply(f3, foot, count, B, S, T)
    return FssLossFn.apply(low, prob, B, HL, WL, HS, WS, lab, ALPHA)


def tail_times(reps, inner):
    f3, low, mask, lab = episode_tensors()
    f3.requires_grad_()
    low.requires_grad_()
    tails = {"fused": fused_tail, "composed": composed_tail}
    times, peak, loss = {k: [] for k in tails}, {}, {}
    for it in range(reps + 3):
        for name, fn in tails.items():  # alternate the two inside one process
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                out = fn(f3, low, mask, lab)
                torch.autograd.grad(out, [f3, low])
            e1.record()
            e1.synchronize()
            if it >= 3:
                times[name].append(e0.elapsed_time(e1) / inner)
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            loss[name] = out.item()
    res = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
               "peak_MiB": round(peak[k], 1), "loss": loss[k]} for k, v in times.items()}
    res["composed_over_fused"] = round(res["composed"]["median_ms"] / res["fused"]["median_ms"], 2)
    return res


def step_time(reps):
    from dformer_amd.segmentor import EncoderDecoder
    from dformer_amd.train import FusedAdamW, meta_train_step
    cfg = bench.make_cfg("DFormer-Base", "ham")
    cfg.update(backbone="DFormerTrav-Base", num_classes=2, alpha=ALPHA, temperature=T)
    torch.manual_seed(0)
    m = EncoderDecoder(cfg=cfg).to(DEV).set_compute_dtype(torch.bfloat16).train()
    m.return_logits = False
    opt = FusedAdamW(m, lr=cfg.lr, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
    _, _, mask, lab = episode_tensors()
    n = B * S + B
    rgb = torch.randn(n, 3, H, W, device=DEV)
    scan = torch.rand(n, 1, 360, device=DEV) * 9.5 + 0.5
    ep = (rgb[:B * S].view(B, S, 3, H, W), scan[:B * S].view(B, S, 1, 360), mask.view(B, S, H, W), rgb[B * S:],
          scan[B * S:], lab)
    for _ in range(3):
        meta_train_step(m, opt, *ep)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        meta_train_step(m, opt, *ep)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2),
            "peak_allocated_MiB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "images_per_step": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="tail runs per timed region")
    ap.add_argument("--no-step", action="store_true", help="kernels and tails only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "episode": dict(B=B, S=S, H=H, W=W, stage3=[HS, WS, C], low=[HL, WL]),
           "reps": a.reps, "kernels": kernel_times(a.reps), "runs_per_timed_region": a.inner,
           "tail_fwd_bwd": tail_times(a.reps, a.inner)}
    if not a.no_step:
        res["meta_train_step_eager"] = step_time(a.reps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
