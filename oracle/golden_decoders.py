"""Decoder fixtures: the reference's NMF2D, LightHamHead, MLP DecoderHead, FCNHead and UPerHead alone, in float64.

The heads run in train mode with BN eps 1e-3 / momentum 0.1 (what init_func.py:11-15 gives them inside the
segmentor) and without dropout. ham / fcnhead / uperhead draw their inputs under "<name>#<seed>", the first seed
whose ReLU inputs all stay more than margin x max away from zero: the HIP fp32 path then sees the same activation
pattern as fp64 and every gradient behind a ReLU can be gated tightly. fcnhead / uperhead also store
env_bf16/y and env_f16/y: the rel-to-max output error of the reference itself in float32 under torch.autocast.
"""
import numpy as np
import torch
import torch.nn as nn

import gen
from golden_common import (BN, f32, ham_relus, load_weights, module_relus, out_of_place_laterals, param_grads, ref,
                           rel, relu_margin, running_stats, save, search_seed, set_bn, t)


def golden_nmf(name, B, C, H, W, train=True):
    nmf = ref().ham.NMF2D(dict(device="cpu"))
    nmf.train(train)
    bases = gen.nmf_bases(B, C, 64, name=name + "/bases")
    nmf._build_bases = lambda B_, S, D, R, cuda=False: torch.from_numpy(bases.copy())
    x = t(gen.uniform(name + "/x", (B, C, H, W)))
    y = nmf(x)
    gy = gen.normal(name + "/gy", y.shape)
    (y * t(gy, False)).sum().backward()
    save(name, y=y.detach().numpy().astype(np.float32), gx=x.grad.numpy().astype(np.float32),
         meta=np.array([B, C, H, W, int(train)]))


def _head(head, dtype=torch.float64):
    set_bn(head)
    load_weights(head)
    return head.to(dtype).train()


def _autocast_env(make32, xs, y64):
    """env_bf16/y, env_f16/y of a fresh float32 head on the inputs xs (float64 arrays)."""
    env = {}
    for key, dt in (("env_bf16/y", torch.bfloat16), ("env_f16/y", torch.float16)):
        with torch.no_grad(), torch.autocast("cpu", dtype=dt):
            ya = make32()([f32(x) for x in xs])
        env[key] = np.array(rel(ya.double().numpy(), y64))
        print(f"    {key} {float(env[key]):.3e}")
    return env


def golden_ham(name, in_ch, B, H, W, ncls=40, margin=1e-5, tries=400):
    """Stored: y, gf1..3, parameter gradients, running statistics, margin, meta = [B, H, W, ncls, train, seed, *in_ch]."""
    head = ref().ham.LightHamHead(in_channels=in_ch, num_classes=ncls, in_index=[1, 2, 3], norm_cfg=BN,
                                  channels=512, device="cpu")
    head.dropout = None
    head = _head(head)

    def draw(s, grad):
        tag = f"{name}#{s}"
        bases = gen.nmf_bases(B, 512, 64, name=tag + "/bases")
        head.hamburger.ham._build_bases = lambda B_, S, D, R, cuda=False: torch.from_numpy(bases.copy())
        return [None] + [t(gen.normal(tag + f"/f{i}", (B, c, H >> i, W >> i)), grad) for i, c in enumerate(in_ch)]

    s, mg = search_seed(lambda s: relu_margin(head, lambda: head(draw(s, False)), ham_relus(head)), range(tries), margin)
    print(f"  {name}: input seed {s}, ReLU margin {mg:.2e}")
    feats = draw(s, True)
    y = head(feats)
    gy = gen.normal(f"{name}#{s}/gy", y.shape)
    (y * t(gy, False)).sum().backward()
    save(name, y=y.detach().numpy().astype(np.float32),
         **{f"gf{i}": f.grad.numpy().astype(np.float32) for i, f in enumerate(feats) if i},
         meta=np.array([B, H, W, ncls, 1, s] + list(in_ch)), margin=np.array(mg),
         **param_grads(head), **running_stats(head))


def golden_mlpdec(name, in_ch, B, H, W, embed, ncls=40):
    head = ref().mlpdec.DecoderHead(in_channels=in_ch, num_classes=ncls, norm_layer=nn.BatchNorm2d, embed_dim=embed)
    head.dropout = nn.Identity()
    head = _head(head)
    sizes = [(H, W)]
    for _ in range(3):
        h, w = sizes[-1]
        sizes.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
    feats = [t(gen.normal(name + f"/f{i}", (B, c, *sizes[i]))) for i, c in enumerate(in_ch)]
    y = head(feats)
    gy = gen.normal(name + "/gy", y.shape)
    (y * t(gy, False)).sum().backward()
    save(name, y=y.detach().numpy().astype(np.float32),
         **{f"gf{i}": f.grad.numpy().astype(np.float32) for i, f in enumerate(feats)},
         meta=np.array([B, H, W, ncls, embed] + list(in_ch)), **param_grads(head))


def golden_fcnhead(name, B, cin, hidden, H, W, margin=1e-5, tries=400):
    """FCNHead(cin, hidden) (models/decoders/fcnhead.py:9-29; builder.py:143 binds cfg.num_classes to the hidden
    width and leaves the output 40 wide). Stored: y, gx, every parameter gradient in full, running statistics,
    margin, meta = [B, cin, hidden, H, W, seed], env_bf16/y, env_f16/y."""
    make = lambda dtype=torch.float32: _head(ref().fcnhead.FCNHead(cin, hidden, norm_layer=nn.BatchNorm2d), dtype)  # noqa: E731
    head = make(torch.float64)
    draw = lambda s: gen.normal(f"{name}#{s}/x", (B, cin, H, W))  # noqa: E731
    s, mg = search_seed(lambda s: relu_margin(head, lambda: head(t(draw(s), False)), module_relus(head)),
                        range(tries), margin)
    print(f"  {name}: input seed {s}, ReLU margin {mg:.2e}")
    x = t(draw(s))
    y = head(x)
    assert y.shape == (B, 40, H, W)
    gy = gen.normal(f"{name}#{s}/gy", y.shape)
    (y * t(gy, False)).sum().backward()
    y64 = y.detach().numpy()
    save(name, y=y64.astype(np.float32), gx=x.grad.numpy().astype(np.float32), margin=np.array(mg),
         meta=np.array([B, cin, hidden, H, W, s]), **param_grads(head, big=np.inf), **running_stats(head),
         **_autocast_env(lambda: (lambda xs: make()(xs[0])), [draw(s)], y64))


def golden_uperhead(name, B, in_ch, channels, sizes, margin, tries=400):
    """UPerHead(in_ch, channels) (models/decoders/UPernet.py:8-146) with its 12 ReLUs watched and the in-place
    top-down sum routed around (golden_common.out_of_place_laterals). Stored: y, gx/<i>, parameter gradients
    (tensors of more than 100,000 elements as gradfp/), running statistics, margin, meta = [B, channels, seed],
    shapes = [[C, H, W]] per input, env_bf16/y, env_f16/y."""
    def make(dtype=torch.float32):
        head = ref().uper.UPerHead(list(in_ch), num_classes=40, channels=channels, norm_layer=nn.BatchNorm2d)
        out_of_place_laterals(head)
        return _head(head, dtype)

    head = make(torch.float64)
    assert len(module_relus(head)) == 12
    draw = lambda s: [gen.normal(f"{name}#{s}/x{i}", (B, c, h, w)) for i, (c, (h, w)) in enumerate(zip(in_ch, sizes))]  # noqa: E731
    s, mg = search_seed(lambda s: relu_margin(head, lambda: head([t(a, False) for a in draw(s)]), module_relus(head)),
                        range(tries), margin)
    print(f"  {name}: input seed {s}, ReLU margin {mg:.2e}")
    xs = [t(a) for a in draw(s)]
    y = head(xs)
    assert y.shape == (B, 40) + tuple(sizes[0])
    gy = gen.normal(f"{name}#{s}/gy", y.shape)
    (y * t(gy, False)).sum().backward()
    y64 = y.detach().numpy()
    save(name, y=y64.astype(np.float32), margin=np.array(mg), meta=np.array([B, channels, s]),
         shapes=np.array([[c, h, w] for c, (h, w) in zip(in_ch, sizes)]), **param_grads(head, big=100_000),
         **running_stats(head), **{f"gx/{i}": x.grad.numpy().astype(np.float32) for i, x in enumerate(xs)},
         **_autocast_env(make, draw(s), y64))
