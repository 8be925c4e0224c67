"""Generate tests/golden/fcnhead_*.npz and e2e_tiny_aux*.npz: the reference's auxiliary FCNHead
(models/decoders/fcnhead.py:9-29) alone, and DFormer-Tiny + ham trained with aux_rate = 0.4
(models/builder.py:138-143, 204-207, 231-232), on CPU in float64.

TEST INFRASTRUCTURE. Run in the build container only (it needs the read-only reference that
oracle/ref_import.py imports):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_aux_goldens.py [name prefix ...]
It reuses oracle/make_goldens.py's weights, inputs, `e2e_forward` and `save`; nothing under oracle/
changes and nothing of the reference is copied: the files hold arrays and name lists only (inputs come
from the seeds in gen.py).

fcnhead_<name>: FCNHead(Cin, hidden) in train mode (BN eps 1e-3, momentum 0.1 as init_func.py:11-13 sets
them), input gen.normal("<name>#<seed>/x"), upstream gradient gen.normal("<name>#<seed>/gy") on the 40-wide
output. The input seed is the first one whose ReLU inputs all stay >= 1e-5 x max away from zero (the
rule of make_goldens.golden_ham). Stored: y, gx, every parameter gradient in full (grad/<key>), the BN
running statistics after the step (buf/<key>), margin, meta = [B, Cin, hidden, H, W, seed], and
env_bf16/y, env_f16/y: the rel-to-max output error of the reference itself in float32 under
torch.autocast(bfloat16 / float16) on the same input.

e2e_tiny_aux / e2e_tiny_aux37: the inputs of e2e_tiny_small (2 x 64x96, bases "e2e_tiny_small/bases", its
input seed meta[4]) with aux_rate = 0.4 and num_classes 40 / 37. builder.py:143 binds cfg.num_classes to
FCNHead's hidden width and leaves its num_classes at 40, so aux_low is [2, 40, 4, 6] in both. With 40
classes the main path is e2e_tiny_small's: `low` and the main loss are asserted equal to that golden to
float32 rounding. Stored: aux_low, loss_main, loss_aux, loss, gfp/<key> (16-sample fingerprints of every
parameter gradient of the total loss), auxgrad/<key> (the aux head's gradients in full), env/... (the
reference's own float32 error, as make_goldens.golden_bf16_env(dtype=None) forms it), margin (the aux
ReLU's), sd_keys / sd_shapes (state_dict keys in order, shapes as "a,b,c"), gw_decay / gw_nodecay (the
parameter names of utils/init_func.py group_weight's two groups in order), meta = [B, H, W, ncls, seed].
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen  # noqa: E402
import make_goldens as MG  # noqa: E402  (sets the default dtype to float64 and imports the reference)

AUX_RATE = 0.4


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _fcn_head(cin, hidden, dtype=torch.float64):
    import models.decoders.fcnhead as fcn  # noqa: E402  (the reference, read-only)
    head = fcn.FCNHead(cin, hidden, norm_layer=nn.BatchNorm2d)
    head.conv[1].eps, head.conv[1].momentum = 1e-3, 0.1
    MG.load_weights(head)
    return head.to(dtype).train()


def _relu_margin(head, x):
    """min |ReLU input| / max |ReLU input| of the head's one ReLU, running statistics left untouched."""
    seen = {}
    h = head.conv[2].register_forward_pre_hook(lambda m, a: seen.__setitem__("z", a[0].detach().clone()))
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    with torch.no_grad():
        head(x)
    head.load_state_dict(sd)
    h.remove()
    z = seen["z"].abs()
    return (z.min() / z.max()).item()


def golden_fcnhead(name, B, cin, hidden, H, W, margin=1e-5, tries=400):
    head = _fcn_head(cin, hidden)
    for s in range(tries):
        tag = f"{name}#{s}"
        mg = _relu_margin(head, MG.t(gen.normal(tag + "/x", (B, cin, H, W)), False))
        if mg >= margin:
            break
    else:
        raise RuntimeError(f"no input seed with ReLU margin >= {margin}")
    print(f"  {name}: input seed {s}, ReLU margin {mg:.2e}")
    x = MG.t(gen.normal(tag + "/x", (B, cin, H, W)))
    y = head(x)
    assert y.shape == (B, 40, H, W)
    gy = gen.normal(tag + "/gy", y.shape)
    (y * MG.t(gy, False)).sum().backward()
    arrays = {"grad/" + n: p.grad.numpy().astype(np.float32) for n, p in head.named_parameters()}
    for n, b in head.named_buffers():
        if "running" in n:
            arrays["buf/" + n] = b.numpy().astype(np.float32)
    y64 = y.detach().numpy()
    for key, dt in (("env_bf16/y", torch.bfloat16), ("env_f16/y", torch.float16)):
        h32 = _fcn_head(cin, hidden, torch.float32)
        with torch.no_grad(), torch.autocast("cpu", dtype=dt):
            ya = h32(torch.from_numpy(gen.normal(tag + "/x", (B, cin, H, W))).float())
        arrays[key] = np.array(_rel(ya.double().numpy(), y64))
        print(f"  {name}: {key} {float(arrays[key]):.3e}")
    MG.save(name, y=y64.astype(np.float32), gx=x.grad.numpy().astype(np.float32), margin=np.array(mg),
            meta=np.array([B, cin, hidden, H, W, s]), **arrays)


def _build_aux(ncls, dtype=torch.float64):
    cfg = MG.Cfg(backbone="DFormer-Tiny", decoder="ham", decoder_embed_dim=512, num_classes=ncls,
                 drop_path_rate=0.0, aux_rate=AUX_RATE, device="cpu", pretrained_model=None, bn_eps=1e-3,
                 bn_momentum=0.1, background=255)
    crit = nn.CrossEntropyLoss(reduction="none", ignore_index=255)
    model = MG.builder.EncoderDecoder(cfg=cfg, criterion=crit, norm_layer=nn.BatchNorm2d, syncbn=False)
    model.decode_head.dropout = None
    MG.load_weights(model)
    return model.to(dtype).train(), cfg


def _aux_step(model, cfg, rgb, dep, lab, bases):
    """builder.py:193-208, 224-233 with the HEAD tuple bug routed around (MG.e2e_forward)."""
    seen = {}
    h = model.aux_head.conv[2].register_forward_pre_hook(lambda m, a: seen.__setitem__("z", a[0].detach().clone()))
    feats, low, out = MG.e2e_forward(model, rgb, dep, bases)
    aux_low = model.aux_head(feats[model.aux_index])
    h.remove()
    aux = F.interpolate(aux_low, size=rgb.shape[2:], mode="bilinear", align_corners=False)
    valid = lab != cfg.background
    loss_main = model.criterion(out.to(rgb.dtype), lab)[valid].mean()
    loss_aux = model.criterion(aux.to(rgb.dtype), lab)[valid].mean()
    loss = loss_main + model.aux_rate * loss_aux
    z = seen["z"].abs()
    return low, aux_low, loss_main, loss_aux, loss, (z.min() / z.max()).item()


def golden_e2e_aux(name, ncls, base="e2e_tiny_small", margin=3e-6):
    t0 = time.time()
    g0 = dict(np.load(os.path.join(MG.OUT, base + ".npz")))
    B, H, W = [int(v) for v in g0["meta"][:3]]
    seed = int(g0["meta"][4])
    rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=seed)
    lab = torch.from_numpy(gen.labels(B, H, W, ncls)).long()
    bases = gen.nmf_bases(B, 512, 64, name=base + "/bases")
    model, cfg = _build_aux(ncls)
    low, aux_low, loss_main, loss_aux, loss, mg = _aux_step(model, cfg, MG.t(rgb_np, False), MG.t(dep_np, False),
                                                            lab, bases)
    assert tuple(aux_low.shape) == (B, 40, H // 16, W // 16), aux_low.shape
    assert mg > margin, f"aux ReLU margin {mg:.3e} <= {margin}"
    print(f"  {name}: aux ReLU margin {mg:.2e}, main loss {loss_main.item():.6f}, aux loss {loss_aux.item():.6f}")
    if ncls == int(g0["meta"][3]):  # the main path is the existing golden's
        dlow = np.abs(low.detach().numpy() - g0["low"].astype(np.float64)).max()
        print(f"  {name}: max |low - {base}.low| {dlow:.2e}, main loss - golden {loss_main.item() - float(g0['loss']):.2e}")
        assert dlow < 2e-7 * max(np.abs(g0["low"]).max(), 1.0)
        assert abs(loss_main.item() - float(g0["loss"])) < 1e-12 * abs(float(g0["loss"])) + 1e-15
    loss.backward()
    arrays = {"gfp/" + n: gen.fingerprint(p.grad.numpy(), 16) for n, p in model.named_parameters()
              if p.grad is not None}
    for n, p in model.aux_head.named_parameters():
        arrays["auxgrad/aux_head." + n] = p.grad.numpy().astype(np.float32)
    sd = model.state_dict()
    arrays["sd_keys"] = np.array(list(sd.keys()))
    arrays["sd_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    from utils.init_func import group_weight  # noqa: E402  (the reference, read-only)
    groups = group_weight([], model, nn.BatchNorm2d, 6e-5)
    ids = {id(p): n for n, p in model.named_parameters()}
    arrays["gw_decay"] = np.array([ids[id(p)] for p in groups[0]["params"]])
    arrays["gw_nodecay"] = np.array([ids[id(p)] for p in groups[1]["params"]])
    # the reference's own float32 error on the same step (make_goldens.golden_bf16_env(dtype=None))
    m32, _ = _build_aux(ncls, torch.float32)
    r32 = _aux_step(m32, cfg, torch.from_numpy(rgb_np).float(), torch.from_numpy(dep_np).float(), lab,
                    bases.astype(np.float32))
    r32[4].backward()
    arrays["env/aux_low"] = np.array(_rel(r32[1].detach().double().numpy(), aux_low.detach().numpy()))
    arrays["env/loss"] = np.array(abs(r32[4].item() - loss.item()) / abs(loss.item()))
    for n, p in m32.named_parameters():
        if p.grad is not None and "gfp/" + n in arrays:
            arrays["env/gfp/" + n] = np.array(MG._fp_rel_err(gen.fingerprint(p.grad.double().numpy(), 16),
                                                             arrays["gfp/" + n], atol=1e-4))
    gv = np.array([v for k, v in arrays.items() if k.startswith("env/gfp/")])
    print(f"  {name}: fp32 envelope aux_low {float(arrays['env/aux_low']):.3e} loss {float(arrays['env/loss']):.3e} "
          f"param-grad median {np.median(gv):.3e} max {gv.max():.3e}")
    MG.save(name, aux_low=aux_low.detach().numpy().astype(np.float32), loss_main=np.array(loss_main.item()),
            loss_aux=np.array(loss_aux.item()), loss=np.array(loss.item()), margin=np.array(mg),
            meta=np.array([B, H, W, ncls, seed]), **arrays)
    print(f"  {name}: {time.time() - t0:.1f}s")


def main():
    which = sys.argv[1:]
    torch.manual_seed(0)

    def want(n):
        return not which or any(n.startswith(w) for w in which)

    if want("fcnhead_c128"):
        golden_fcnhead("fcnhead_c128", 2, 128, 37, 5, 7)
    if want("fcnhead_c288"):
        golden_fcnhead("fcnhead_c288", 1, 288, 40, 3, 2)  # every pixel on the border
    if want("e2e_tiny_aux37"):
        golden_e2e_aux("e2e_tiny_aux37", 37)
    if want("e2e_tiny_aux"):
        golden_e2e_aux("e2e_tiny_aux", 40)


if __name__ == "__main__":
    main()
