"""Evaluation fixtures: the reference's own evaluate_msf (msf_*), evaluate_msf(sliding=True) (slide_*) and
single-scale evaluate (eval_*) of utils/val_mm.py, on CPU in float64 with the model in eval mode.

Two batches (input and label seeds 8964, 8965): the reference divides by int(len(loader) * 0.5). The model is
wrapped so that encode_decode's HEAD tuple bug is routed around (golden_common.e2e_forward; NMF bases injected),
and val_mm.Metrics is replaced for the run by a subclass that records what reaches Metrics.update.
"""
import numpy as np
import torch
import torch.nn as nn

import gen
from golden_common import Cfg, build_segmentor, e2e_forward, e2e_seeds, ref, save


def _reference_eval(name, backbone, B, H, W, decoder, ncls, embed, run, depth_key="modal_x", fns=1, **config):
    """(metrics, what Metrics.update received per batch, the model's full-resolution logits per forward) of
    run(val_mm, model, loader, config, device, engine)."""
    val_mm = ref().val_mm
    model, _ = build_segmentor(backbone, decoder, ncls, embed)
    model.eval()
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases") if decoder == "ham" else None
    captured, logits = [], []

    class Wrapped(nn.Module):
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, rgb, dep):
            out = e2e_forward(self.m, rgb, dep, bases)[2]
            logits.append(out.detach().clone())
            return out

    class RecMetrics(val_mm.Metrics):
        def update(self, pred, target):
            captured.append(pred.detach().clone())
            super().update(pred, target)

    loader = []
    for s in e2e_seeds(2):
        rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=s)
        loader.append({"rgb": torch.from_numpy(rgb_np), depth_key: torch.from_numpy(dep_np),
                       "gt": torch.from_numpy(gen.labels(B, H, W, ncls, seed=s)).long(), "fn": ["x.png"] * fns})
    config = Cfg(num_classes=ncls, background=255, dataset_name="NYUDepthv2", **config)
    real, val_mm.Metrics = val_mm.Metrics, RecMetrics
    try:
        with torch.no_grad():
            metrics = run(val_mm, Wrapped(), loader, config, torch.device("cpu"), Cfg(distributed=False, local_rank=0))
    finally:
        val_mm.Metrics = real
    return metrics, captured, logits


def golden_msf(name, backbone, B, H, W, decoder="ham", ncls=40, embed=512, scales=(0.75, 1.0, 1.25), flip=True):
    """evaluate_msf (utils/val_mm.py:325-472): the summed softmax scores handed to Metrics.update per batch and
    the final confusion histogram."""
    metrics, captured, _ = _reference_eval(
        name, backbone, B, H, W, decoder, ncls, embed,
        lambda vm, model, loader, config, dev, engine: vm.evaluate_msf(model, loader, config, dev, list(scales), flip, engine))
    save(name, scores0=captured[0].numpy().astype(np.float32), scores1=captured[1].numpy().astype(np.float32),
         hist=metrics.hist.numpy(), scales=np.array(scales), meta=np.array([B, H, W, ncls, int(flip)]))


BAND = 2e-3  # tests/test_predict_gpu.py: a pixel may differ where gap <= BAND * amax


def golden_eval(name, backbone, B, H, W, decoder, ncls, embed):
    """evaluate (utils/val_mm.py:102-207; batch keys rgb, laser, gt, fn). Per batch i: `pred{i}`, the uint8 argmax
    of what reached Metrics.update, and `gap{i}` (float32), the top-1 minus top-2 of the float64 full-resolution
    logits per pixel: a float32 run may only disagree with pred{i} where the gap is within its own error. `amax`
    is max |logit| over both batches, `hist` the final confusion histogram, `meta` = [B, H, W, ncls]."""
    metrics, captured, logits = _reference_eval(
        name, backbone, B, H, W, decoder, ncls, embed, depth_key="laser", fns=B,
        run=lambda vm, model, loader, config, dev, engine: vm.evaluate(model, loader, config, dev, engine))
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
    save(name, hist=metrics.hist.numpy(), amax=np.array(amax), meta=np.array([B, H, W, ncls]), **arrays)
    print(f"  {name}: max |logit| {amax:.4f}; {near} of {npix} pixels ({near / npix:.2%}) have gap <= {BAND} * amax")


class _RecordPad:
    """Stands in for val_mm's `F`: records the padding slide_inference gives every crop's logits."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        return getattr(self._real, name)

    def pad(self, x, pad, *a, **k):
        out = self._real.pad(x, pad, *a, **k)
        H, W = out.shape[-2:]
        self._calls[-1].append((H, W, pad[2], H - pad[3], pad[0], W - pad[1]))
        return out


def golden_slide(name, backbone, B, H, W, decoder, ncls, embed, crop, rate, scales, flip=True):
    """evaluate_msf(..., sliding=True) (utils/val_mm.py:257-322, 325-472). Stored: the summed softmax scores of
    batch 0 (float32; `scores0_img<i>`, image 0 in <name>.npz and image i in <name>_img<i>.npz so that every file
    stays small), the confusion histogram over both batches, `scales`, `meta` = [B, H, W, ncls, flip], `crop`,
    `rate`, and per scale k the size the windows were cut from (`size{k}`, after the reference's up-sizing to the
    crop) and the (start, end) of its windows per axis (`win_h{k}`, `win_w{k}`), read off the padding the
    reference applied to every crop's logits."""
    calls = []

    def run(vm, model, loader, config, dev, engine):
        real = dict(F=vm.F, slide_inference=vm.slide_inference)

        def slide_inference(*a, **k):
            calls.append([])
            return real["slide_inference"](*a, **k)

        vm.F, vm.slide_inference = _RecordPad(vm.F, calls), slide_inference
        try:
            return vm.evaluate_msf(model, loader, config, dev, list(scales), flip, engine, sliding=True)
        finally:
            vm.F, vm.slide_inference = real["F"], real["slide_inference"]

    metrics, captured, _ = _reference_eval(name, backbone, B, H, W, decoder, ncls, embed, run,
                                           eval_crop_size=list(crop), eval_stride_rate=rate)
    per_scale = 2 if flip else 1
    assert len(calls) == 2 * per_scale * len(scales), len(calls)
    wins = {}
    for k in range(len(scales)):
        e = calls[k * per_scale]  # batch 0, not flipped
        assert all(c == e for c in calls[k * per_scale:(k + 1) * per_scale]), "flip changes no window"
        wg = sum(1 for r in e if r[2:4] == e[0][2:4])
        hg = len(e) // wg
        wins[f"size{k}"] = np.array(e[0][:2])
        wins[f"win_h{k}"] = np.array([e[i * wg][2:4] for i in range(hg)])
        wins[f"win_w{k}"] = np.array([e[j][4:6] for j in range(wg)])
        print(f"  {name} scale {scales[k]}: {tuple(e[0][:2])} -> {hg} x {wg} windows")
    scores = captured[0].numpy().astype(np.float32)
    save(name, scores0_img0=scores[0], hist=metrics.hist.numpy(), scales=np.array(scales),
         meta=np.array([B, H, W, ncls, int(flip)]), crop=np.array(crop), rate=np.array(rate), **wins)
    for i in range(1, B):
        save(f"{name}_img{i}", **{f"scores0_img{i}": scores[i]})
