"""Generate tests/golden/slide_*.npz: the reference's own evaluate_msf(..., sliding=True)
(utils/val_mm.py:257-322, 325-472) on CPU in float64.

TEST INFRASTRUCTURE. Run in the build container only (it needs the read-only reference that
oracle/ref_import.py imports):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_slide_goldens.py [name prefix ...]
It reuses oracle/make_goldens.py's model construction (`build_segmentor`, `e2e_forward`), its `save`
and its way of capturing what evaluate_msf hands to Metrics.update; nothing under oracle/ changes and
nothing of the reference is copied: the files hold arrays only (inputs come from the seeds in gen.py).

Each fixture stores the summed softmax scores of batch 0 (float32; `scores0`, split per image into
`<name>.npz` and `<name>_img<i>.npz` so that every file stays small), the confusion histogram over both
batches, `scales`, `meta` = [B, H, W, ncls, flip], `crop`, `rate`, and per scale k the size the windows
were cut from (`size{k}`, after the reference's up-sizing to the crop) and the (start, end) of its windows
per axis (`win_h{k}`, `win_w{k}`), read off the padding the reference applied to every crop's logits.
Two batches (seeds 8964, 8965): the reference divides by int(len(loader) * 0.5).
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
    import utils.val_mm as val_mm  # noqa: E402  (the reference, read-only)
    t0 = time.time()
    model, _ = MG.build_segmentor(backbone, decoder, ncls, embed)
    model.eval()
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases") if decoder == "ham" else None

    class Wrapped(nn.Module):
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, rgb, dep):
            return MG.e2e_forward(self.m, rgb, dep, bases)[2]

    captured, calls = [], []

    class RecMetrics(val_mm.Metrics):
        def update(self, pred, target):
            captured.append(pred.detach().clone())
            super().update(pred, target)

    real = dict(Metrics=val_mm.Metrics, F=val_mm.F, slide_inference=val_mm.slide_inference)

    def slide_inference(*a, **k):
        calls.append([])
        return real["slide_inference"](*a, **k)

    val_mm.Metrics, val_mm.F, val_mm.slide_inference = RecMetrics, _RecordPad(val_mm.F, calls), slide_inference
    loader = []
    for i in range(2):
        rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=8964 + i)
        loader.append({"rgb": torch.from_numpy(rgb_np), "modal_x": torch.from_numpy(dep_np),
                       "gt": torch.from_numpy(gen.labels(B, H, W, ncls, seed=8964 + i)).long(), "fn": ["x.png"]})
    config = MG.Cfg(num_classes=ncls, background=255, dataset_name="NYUDepthv2", eval_crop_size=list(crop),
                    eval_stride_rate=rate)
    engine = MG.Cfg(distributed=False, local_rank=0)
    try:
        with torch.no_grad():
            metrics = val_mm.evaluate_msf(Wrapped(), loader, config, torch.device("cpu"), list(scales), flip, engine,
                                          sliding=True)
    finally:
        for k, v in real.items():
            setattr(val_mm, k, v)
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
    MG.save(name, scores0_img0=scores[0], hist=metrics.hist.numpy(), scales=np.array(scales),
            meta=np.array([B, H, W, ncls, int(flip)]), crop=np.array(crop), rate=np.array(rate), **wins)
    for i in range(1, B):
        MG.save(f"{name}_img{i}", **{f"scores0_img{i}": scores[i]})
    print(f"  {name}: {time.time() - t0:.1f}s")


def main():
    which = sys.argv[1:]
    torch.manual_seed(0)
    cases = [
        # 1x2, 2x2 and 3x4 window grids, the last row / column of windows clamped
        ("slide_tiny_ham", "DFormer-Tiny", 2, 70, 90, "ham", 40, 512, (64, 64), 2 / 3, (0.75, 1.0, 1.5)),
        # scales 0.5 and 1.0 are smaller than the crop (1.0: 64x64 -> 64x96 changes the aspect ratio);
        # 1.75 gives a 2x2 grid
        ("slide_tiny_mlp", "DFormer-Tiny", 1, 45, 61, "MLPDecoder", 37, 64, (64, 96), 0.5, (0.5, 1.0, 1.75)),
    ]
    for c in cases:
        if not which or any(c[0].startswith(w) for w in which):
            golden_slide(*c)


if __name__ == "__main__":
    main()
