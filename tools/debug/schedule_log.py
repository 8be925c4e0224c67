"""Log the stream schedule of one eager training step, to compare two checkouts line for line.

    python tools/debug/schedule_log.py OUT_DIR

DFormer-Tiny, 2 x 64 x 96, bf16, eager; each decoder (ham, MLPDecoder) with kernels.WG_STREAM_MIN_FLOPS at
its default and at 0 (every weight-gradient group on its own stream): four logs OUT_DIR/<decoder>_<wg>.log.
Two warm-up steps, then the third step is logged:
    L <entry point> <stream>     a library call returned (kernels.check), on the then-current stream
    W <waiter> <waited>          Stream.wait_stream
    R <stream> <count>           Tensor.record_stream calls per stream (totals, at the end)
Streams are numbered by first appearance among the L / W lines. Prints one sha256 per log: equal digests
mean the same launches and waits in the same order and the same record_stream counts. Uses only names that
are stable across refactors of the stream code (kernels.check, kernels.WG_STREAM_MIN_FLOPS, train_step).
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from dformer_amd import kernels as K  # noqa: E402
from dformer_amd.segmentor import EncoderDecoder  # noqa: E402
from dformer_amd.train import FusedAdamW, train_step  # noqa: E402


def logged_step(step):
    lines, ordinal, records = [], {}, {}

    def num(s):
        return ordinal.setdefault(s.cuda_stream, len(ordinal))

    check, wait, record = K.check, torch.cuda.Stream.wait_stream, torch.Tensor.record_stream

    def check_(status, what):
        lines.append(f"L {what} {num(torch.cuda.current_stream())}")
        return check(status, what)

    def wait_(self, other):
        lines.append(f"W {num(self)} {num(other)}")
        return wait(self, other)

    def record_(self, s):
        records[s.cuda_stream] = records.get(s.cuda_stream, 0) + 1
        return record(self, s)

    K.check, torch.cuda.Stream.wait_stream, torch.Tensor.record_stream = check_, wait_, record_
    try:
        step()
        torch.cuda.synchronize()
    finally:
        K.check, torch.cuda.Stream.wait_stream, torch.Tensor.record_stream = check, wait, record
    for n, c in sorted((ordinal.get(h, -1), c) for h, c in records.items()):
        lines.append(f"R {n} {c}")
    return lines


def main(out):
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda", 0)
    default = K.WG_STREAM_MIN_FLOPS
    for decoder in ("ham", "MLPDecoder"):
        for tag, wg in (("default", default), ("0", 0)):
            K.WG_STREAM_MIN_FLOPS = wg
            cfg = bench.make_cfg("DFormer-Tiny", decoder)
            torch.manual_seed(3)
            model = EncoderDecoder(cfg=cfg).to(dev).set_compute_dtype(torch.bfloat16)
            model.return_logits = False
            model.train()
            opt = FusedAdamW(model, lr=1e-3, weight_decay=cfg.weight_decay, compute_dtype=torch.bfloat16)
            rgb, dep, lab = bench.synthetic_batch(2, 64, 96, cfg.num_classes, dev, 5)
            for _ in range(2):
                train_step(model, opt, rgb, dep, lab)
            torch.cuda.synchronize()
            lines = logged_step(lambda: train_step(model, opt, rgb, dep, lab))
            text = "\n".join(lines) + "\n"
            with open(os.path.join(out, f"{decoder}_{tag}.log"), "w") as fh:
                fh.write(text)
            nl, nw = sum(ln[0] == "L" for ln in lines), sum(ln[0] == "W" for ln in lines)
            print(f"{decoder}_{tag}: {hashlib.sha256(text.encode()).hexdigest()} "
                  f"({nl} launches, {nw} waits, {len(set(ln.split()[-1] for ln in lines if ln[0] == 'L'))} streams)")
    K.WG_STREAM_MIN_FLOPS = default


if __name__ == "__main__":
    main(sys.argv[1])
