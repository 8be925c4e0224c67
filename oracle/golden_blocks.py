"""Block fixtures: block_*.npz (one reference Block in float64) and bf16env_block_*.npz (its own bf16 error)."""
import numpy as np
import torch

import gen
from golden_common import BN, fp_rel_err, f32, load, load_weights, param_grads, ref, rel, save, t

MODELS = {  # DFormer.py:460-497
    "tiny": dict(dims=[32, 64, 128, 256], heads=[1, 2, 4, 8], ratios=[8, 8, 4, 4], depths=[3, 3, 5, 2]),
    "base": dict(dims=[64, 128, 256, 512], heads=[1, 2, 4, 8], ratios=[8, 8, 4, 4], depths=[3, 3, 12, 2]),
    "large": dict(dims=[96, 192, 288, 576], heads=[1, 2, 4, 8], ratios=[8, 8, 4, 4], depths=[3, 3, 12, 2]),
}


def make_block(model, stage, last=False, drop_prob=0.0):
    m = MODELS[model]
    C = m["dims"][stage]
    depth = m["depths"][stage]
    j = depth - 1 if last else 0
    blk = ref().dformer.Block(index=0, dim=C, num_head=m["heads"][stage], norm_cfg=BN,
                              mlp_ratio=m["ratios"][stage], block_index=depth - j, last_block_index=50,
                              window=0 if stage == 0 else 7,
                              dropout_layer=dict(type="DropPath", drop_prob=drop_prob),
                              drop_depth=(stage == 3 and last))
    load_weights(blk)
    return blk, C


def golden_block(name, model, stage, B, H, W, last=False, drop_prob=0.0, masks=None, with_ye=False):
    """One Block's output, input gradients and parameter gradients (fp64) under a seeded linear loss.
    with_ye (a drop_depth Block): x_e's output (the attention's e_back result, DFormer.py:133, 141-145,
    177-181) is in the loss and stored too, although the encoder discards it after the last Block.
    masks: injected DropPath keep masks, one per DropPath call in the order of Block.forward."""
    blk, C = make_block(model, stage, last, drop_prob)
    blk.train()
    x = t(gen.normal(name + "/x", (B, H, W, C)))
    xe = t(gen.normal(name + "/xe", (B, H, W, C // 2)))
    if masks is not None:
        ref().droppath.INJECTED_MASKS = [torch.tensor(mk, dtype=torch.float64) for mk in masks]
    y, ye = blk(x, xe)
    ref().droppath.INJECTED_MASKS = None
    gy = gen.normal(name + "/gy", y.shape)
    loss = (y * t(gy, False)).sum()
    extra = {}
    if not last or with_ye:
        gye = gen.normal(name + "/gye", ye.shape)
        loss = loss + (ye * t(gye, False)).sum()
        extra["y_e"] = ye.detach().numpy().astype(np.float32)
    loss.backward()
    save(name, y=y.detach().numpy().astype(np.float32), gx=x.grad.numpy().astype(np.float32),
         gxe=x.grad.new_zeros(0).numpy() if xe.grad is None else xe.grad.numpy().astype(np.float32),
         meta=np.array([B, H, W, C, stage, int(last), drop_prob * 1e6]), **extra, **param_grads(blk))


def golden_block_bf16_env(name, model, stage, B, H, W, last=False):
    """The reference Block's OWN bf16 error (float32 weights / inputs under torch.autocast(bfloat16)
    on CPU) against the fp64 golden `name`, per output: y, y_e, gx, gxe and every parameter gradient,
    with the statistics the GPU gates use (rel-to-max for full tensors, tests/goldens.py fp_rel_err
    for fingerprinted ones). tests/test_block_gpu.py gates the HIP bf16 Block at a stated multiple
    of this envelope (a bf16 gate must be per Block and relative to what bf16 can do)."""
    g = load(name)
    blk, C = make_block(model, stage, last)
    blk = blk.float().train()
    x = f32(gen.normal(name + "/x", (B, H, W, C))).requires_grad_()
    xe = f32(gen.normal(name + "/xe", (B, H, W, C // 2))).requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y, ye = blk(x, xe)
    loss = (y.float() * f32(gen.normal(name + "/gy", y.shape))).sum()
    if not last:
        loss = loss + (ye.float() * f32(gen.normal(name + "/gye", ye.shape))).sum()
    loss.backward()
    env = {"env/y": rel(y.detach().double().numpy(), g["y"]), "env/gx": rel(x.grad.double().numpy(), g["gx"])}
    if not last:
        env["env/y_e"] = rel(ye.detach().double().numpy(), g["y_e"])
        env["env/gxe"] = rel(xe.grad.double().numpy(), g["gxe"])
    for n, p in blk.named_parameters():
        if p.grad is None:
            continue
        a = p.grad.detach().double().numpy()
        if "grad/" + n in g:
            b = g["grad/" + n].astype(np.float64)
            if np.abs(b).max() < 1e-12:  # mathematically zero gradient (fp64 noise): not gated
                continue
            env["env/grad/" + n] = rel(a, b)
        elif "gradfp/" + n in g:
            env["env/grad/" + n] = fp_rel_err(gen.fingerprint(a, 256), g["gradfp/" + n])
    gv = np.array([v for k, v in env.items() if k.startswith("env/grad/")])
    print(f"  bf16env {name}: y {env['env/y']:.3e} gx {env['env/gx']:.3e} param-grad median {np.median(gv):.3e} "
          f"max {gv.max():.3e}")
    save("bf16env_" + name, **{k: np.array(v) for k, v in env.items()})
