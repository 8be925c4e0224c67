"""Generate tests/golden/eval_*.npz: the reference's own single-scale evaluate
(utils/val_mm.py:102-207) on CPU in float64.

TEST INFRASTRUCTURE. Run in the build container only (it needs the read-only reference that
oracle/ref_import.py imports):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_eval_goldens.py [name prefix ...]
It reuses oracle/make_goldens.py's model construction (`build_segmentor`, `e2e_forward`) and its `save`;
nothing under oracle/ changes and nothing of the reference is copied: the files hold arrays only
(inputs and labels come from the seeds in gen.py).

Two batches (seeds 8964, 8965; keys rgb, laser, gt, fn): the reference divides by int(len(loader) * 0.5).
Per batch i the fixture stores `pred{i}`, the uint8 argmax of what reached Metrics.update, and `gap{i}`
(float32), the top-1 minus top-2 of the float64 full-resolution logits per pixel: a float32 run may
only disagree with pred{i} where the gap is within its own error. `amax` is max |logit| over both
batches, `hist` the final confusion histogram, `meta` = [B, H, W, ncls].
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen  # noqa: E402
import make_goldens as MG  # noqa: E402  (sets the default dtype to float64 and imports the reference)

BAND = 2e-3  # tests/test_predict_gpu.py: a pixel may differ where gap <= BAND * amax


def golden_eval(name, backbone, B, H, W, decoder, ncls, embed):
    import utils.val_mm as val_mm  # noqa: E402  (the reference, read-only)
    t0 = time.time()
    model, _ = MG.build_segmentor(backbone, decoder, ncls, embed)
    model.eval()
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases") if decoder == "ham" else None
    logits, captured = [], []

    class Wrapped(nn.Module):
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, rgb, dep):
            out = MG.e2e_forward(self.m, rgb, dep, bases)[2]
            logits.append(out.detach().clone())
            return out

    class RecMetrics(val_mm.Metrics):
        def update(self, pred, target):
            captured.append(pred.detach().clone())
            super().update(pred, target)

    loader = []
    for i in range(2):
        rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=8964 + i)
        loader.append({"rgb": torch.from_numpy(rgb_np), "laser": torch.from_numpy(dep_np),
                       "gt": torch.from_numpy(gen.labels(B, H, W, ncls, seed=8964 + i)).long(), "fn": ["x.png"] * B})
    config = MG.Cfg(num_classes=ncls, background=255, dataset_name="NYUDepthv2")
    engine = MG.Cfg(distributed=False, local_rank=0)
    real = val_mm.Metrics
    val_mm.Metrics = RecMetrics
    try:
        with torch.no_grad():
            metrics = val_mm.evaluate(Wrapped(), loader, config, torch.device("cpu"), engine)
    finally:
        val_mm.Metrics = real
    assert len(captured) == len(logits) == 2
    arrays, near, npix = {}, 0, 0
    amax = max(lg.abs().max().item() for lg in logits)
    for i, (pr, lg) in enumerate(zip(captured, logits)):
        pred = pr.argmax(dim=1)
        assert torch.equal(pred, lg.argmax(dim=1)), "the softmax moved an argmax"
        top = lg.topk(2, dim=1).values
        gap = (top[:, 0] - top[:, 1]).numpy()
        arrays[f"pred{i}"] = pred.numpy().astype(np.uint8)
        arrays[f"gap{i}"] = gap.astype(np.float32)
        near += int((gap <= BAND * amax).sum())
        npix += gap.size
    MG.save(name, hist=metrics.hist.numpy(), amax=np.array(amax), meta=np.array([B, H, W, ncls]), **arrays)
    print(f"  {name}: max |logit| {amax:.4f}; {near} of {npix} pixels ({near / npix:.2%}) have gap <= {BAND} * amax")
    print(f"  {name}: {time.time() - t0:.1f}s")


def main():
    which = sys.argv[1:]
    torch.manual_seed(0)
    cases = [
        ("eval_tiny_ham", "DFormer-Tiny", 2, 50, 70, "ham", 40, 512),         # low-res 7x9, x8 head
        ("eval_tiny_mlp", "DFormer-Tiny", 2, 50, 70, "MLPDecoder", 37, 64),   # low-res 13x18, x4 head
    ]
    for c in cases:
        if not which or any(c[0].startswith(w) for w in which):
            golden_eval(*c)


if __name__ == "__main__":
    main()
