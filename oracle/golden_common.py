"""Shared pieces of the golden generators (oracle/golden_*.py, driven by oracle/make_goldens.py).

TEST INFRASTRUCTURE, build container only. Importing this module has no side effects: the read-only
reference is imported, and the default dtype set to float64, by the first call of ref(). Nothing of the
reference is copied: the fixtures hold arrays and name lists only (inputs come from the seeds in gen.py).
"""
import contextlib
import functools
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
# gen / ref_import next to this file; trav_common / fss_common stay in tests/, where the tests import them by name
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "tests")]
import gen  # noqa: E402
import ref_import  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")  # make_goldens.py --out replaces it
BN = dict(type="BN", requires_grad=True)


@functools.lru_cache(None)
def ref():
    """The reference's modules (dformer, ham, mlpdec, builder, droppath, fcnhead, uper, val_mm, init_func)."""
    torch.set_default_dtype(torch.float64)
    dformer, ham, mlpdec, builder, droppath = ref_import.import_ref()
    import models.decoders.fcnhead as fcnhead
    import models.decoders.UPernet as uper
    import utils.init_func as init_func
    import utils.val_mm as val_mm
    return types.SimpleNamespace(dformer=dformer, ham=ham, mlpdec=mlpdec, builder=builder, droppath=droppath,
                                 fcnhead=fcnhead, uper=uper, val_mm=val_mm, init_func=init_func)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_weights(mod, seed=1234):
    sd = mod.state_dict()
    vals = gen.state_dict_values([(k, v.shape) for k, v in sd.items()], seed)
    mod.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})


def t(a, grad=True):
    x = torch.from_numpy(np.asarray(a, dtype=np.float64)).clone()
    return x.requires_grad_(grad)


def f32(a):
    return torch.from_numpy(a).float()


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print(f"  wrote {name}.npz ({os.path.getsize(path) / 1e6:.2f} MB)")


def load(name):
    """A fixture this one is declared to read (golden_registry: `needs`), from the directory being written."""
    return dict(np.load(os.path.join(OUT, name + ".npz")))


def set_bn(mod):
    """init_func.py:11-15 applies cfg.bn_eps / bn_momentum to the decoder; a head built alone gets them here."""
    for m in mod.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eps, m.momentum = 1e-3, 0.1


def running_stats(mod):
    return {"buf/" + n: b.numpy().astype(np.float32) for n, b in mod.named_buffers() if "running" in n}


def inject_bases(model, bases, dtype=torch.float64):
    model.decode_head.hamburger.ham._build_bases = \
        lambda B_, S, D, R, cuda=False: torch.from_numpy(bases.copy()).to(dtype)


# ------------------------------------------------------------------------------- error statistics
def rel(a, b):
    """max |a - b| / max |b|: arrays rel-to-max, scalars (a loss) relative."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def fp_rel_err(fa, fb, atol=1e-9):
    """Same statistic as tests/goldens.py fp_rel_err (sum / abs-sum / l2 / relative L2 of the samples)."""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    return max(abs(fa[0] - fb[0]) / max(fb[1], atol), abs(fa[1] - fb[1]) / max(fb[1], atol),
               abs(fa[2] - fb[2]) / max(fb[2], atol),
               np.linalg.norm(fa[3:] - fb[3:]) / max(np.linalg.norm(fb[3:]), atol))


def lowp_env(golden, low, mod=None, prefix="env/"):
    """The reference's OWN low-precision error (the same step in float32, or float32 under autocast, on CPU),
    which the GPU gates are stated against: rel() of every value in `low` (tensors, arrays or floats by name)
    against `golden`, and for the low-precision module `mod` the fp_rel_err of every parameter gradient's
    16-sample fingerprint against golden["gfp/<key>"], as {prefix + name: 0-d array}."""
    num = lambda v: v.detach().double().numpy() if torch.is_tensor(v) else v  # noqa: E731
    env = {prefix + k: np.array(rel(num(v), num(golden[k]))) for k, v in low.items()}
    for n, p in (mod.named_parameters() if mod is not None else ()):
        if p.grad is not None and "gfp/" + n in golden:
            env[prefix + "gfp/" + n] = np.array(fp_rel_err(gen.fingerprint(p.grad.double().numpy(), 16),
                                                           golden["gfp/" + n], atol=1e-4))
    return env


def env_summary(env):
    gv = np.array([v for k, v in env.items() if k.startswith("env/gfp/")])
    rest = " ".join(f"{k[4:]} {float(v):.3e}" for k, v in env.items() if not k.startswith("env/gfp/"))
    return f"{rest} param-grad median {np.median(gv):.3e} p90 {np.quantile(gv, 0.9):.3e} max {gv.max():.3e}"


# ------------------------------------------------------------------------------- what a fixture stores
def param_grads(mod, big=65536, prefix="grad/", fp=("gradfp/", 256)):
    """Parameter gradients by name: in full (float32, `prefix`) up to `big` elements, as an fp[1]-sample
    gen.fingerprint under fp[0] above. big=0, fp=("gfp/", 16) is what the end-to-end fixtures store."""
    out = {}
    for n, p in mod.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().numpy()
        if g.size > big:
            out[fp[0] + n] = gen.fingerprint(g, fp[1])
        else:
            out[prefix + n] = g.astype(np.float32)
    return out


def gfp(model):
    return param_grads(model, big=0, fp=("gfp/", 16))


def sd_names(model):
    """State-dict keys in order, and their shapes as "a,b,c"."""
    sd = model.state_dict()
    return {"sd_keys": np.array(list(sd.keys())),
            "sd_shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}


def group_names(model):
    """Parameter names of utils/init_func.py group_weight's two groups (decay, no decay), in its order."""
    groups = ref().init_func.group_weight([], model, nn.BatchNorm2d, 6e-5)
    ids = {id(p): n for n, p in model.named_parameters()}
    return [ids[id(p)] for p in groups[0]["params"]], [ids[id(p)] for p in groups[1]["params"]]


def gw_names(model):
    decay, nodecay = group_names(model)
    return {"gw_decay": np.array(decay), "gw_nodecay": np.array(nodecay)}


# ------------------------------------------------------------------------------- ReLU margins and seed search
def ham_relus(head):
    """What relu_margin watches in a LightHamHead: the inputs of the squeeze and align ReLUs, ham_in's output
    (the Hamburger applies F.relu to it) and the Hamburger's relu(x + ham_out)."""
    return [[head.squeeze.activate.register_forward_pre_hook], [head.align.activate.register_forward_pre_hook],
            [head.hamburger.ham_in.register_forward_hook],
            [head.hamburger.register_forward_pre_hook, head.hamburger.ham_out.register_forward_hook]]


def module_relus(mod):
    return [[m.register_forward_pre_hook] for m in mod.modules() if isinstance(m, nn.ReLU)]


def relu_margin(mod, forward, watch):
    """min |z| / max |z| over every watched ReLU input z during the no-grad call forward(). `watch` lists one
    entry per ReLU: the hook registrations (bound register_forward_pre_hook -> that module's input,
    register_forward_hook -> its output) whose tensors sum to z. mod's state dict is restored afterwards: the
    running statistics move in train mode."""
    parts = [[None] * len(w) for w in watch]
    hooks = [reg(lambda m, a, o=None, i=i, j=j: parts[i].__setitem__(j, (a[0] if o is None else o).detach().clone()))
             for i, w in enumerate(watch) for j, reg in enumerate(w)]
    sd = {k: v.clone() for k, v in mod.state_dict().items()}
    with torch.no_grad():
        forward()
    mod.load_state_dict(sd)
    for h in hooks:
        h.remove()
    return min((z.min() / z.max()).item() for z in (sum(p).abs() for p in parts))


def e2e_seeds(tries):
    """The input seeds an end-to-end fixture searches, from gen.rgb_depth's default."""
    return range(8964, 8964 + tries)


def search_seed(margin_of, seeds, margin=None):
    """(seed, margin_of(seed)) of the first seed whose margin exceeds `margin`; with margin=None the best seed."""
    best = (-1.0, None)
    for s in seeds:
        mg = margin_of(s)
        if margin is not None and mg > margin:
            return s, mg
        best = max(best, (mg, s), key=lambda b: b[0])
    if margin is not None:
        raise RuntimeError(f"no input seed with ReLU margin > {margin} (best {best[0]:.2e} at {best[1]})")
    return best[1], best[0]


# ------------------------------------------------------------------------------- the segmentor
def build_segmentor(backbone, decoder="ham", ncls=40, embed=512, aux_rate=0, expand=None, values=None,
                    dtype=torch.float64, **cfg_more):
    """(EncoderDecoder in eval-or-train mode as built, cfg) with deterministic weights and no dropout.
    expand=(N, L, Hout): Trav's attn_expand_e at that size; values=(wseed, ascale): trav_common's weights
    instead of gen.py's; cfg_more: further cfg entries (alpha, temperature)."""
    r = ref()
    cfg = Cfg(backbone=backbone, decoder=decoder, decoder_embed_dim=embed, num_classes=ncls, drop_path_rate=0.0,
              aux_rate=aux_rate, device="cpu", pretrained_model=None, bn_eps=1e-3, bn_momentum=0.1, background=255,
              **cfg_more)
    crit = nn.CrossEntropyLoss(reduction="none", ignore_index=255)
    model = r.builder.EncoderDecoder(cfg=cfg, criterion=crit, norm_layer=nn.BatchNorm2d, syncbn=False)
    if decoder == "UPernet":  # builder.py:145-152 leaves the BN defaults; UPerHead has no dropout
        set_bn(model.decode_head)
        set_bn(model.aux_head)
        out_of_place_laterals(model.decode_head)
    else:
        model.decode_head.dropout = None if decoder == "ham" else nn.Identity()
    if expand is not None:
        model.encoder_backbone.attn_expand_e = r.dformer.Attention1Dto2D(*expand, 64, 4)
    if values is not None:
        import trav_common
        trav_common.load_values(model, *values)
    else:
        load_weights(model)
    return model.to(dtype), cfg


def out_of_place_laterals(head):
    """UPernet.py:80 adds the upsampled coarser level IN PLACE into the lateral Sequential's ReLU output, whose
    backward needs that output, so autograd refuses the training backward. A forward hook returns a clone of
    each lateral's output: the sum lands in the clone, which is the out-of-place sum upstream mmsegmentation
    computes. Forward values are unchanged."""
    for seq in head.lateral_convs:
        seq.register_forward_hook(lambda m, a, o: o.clone())


def e2e_forward(model, rgb, dep, bases=None):
    """encode_decode of builder.py:193-208 with the HEAD tuple bug routed around: the
    DFormer backbones return (outs, None), the Trav backbone the list itself."""
    if bases is not None:
        inject_bases(model, bases, rgb.dtype)
    feats = model.encoder_backbone(rgb, dep)
    feats = feats[0] if isinstance(feats, tuple) else feats
    low = model.decode_head.forward(feats)
    out = F.interpolate(low, size=rgb.shape[-2:], mode="bilinear", align_corners=False)
    return feats, low, out


def train_step(model, cfg, rgb, dep, lab, bases=None, autocast=None, backward=True):
    """One training forward and (unless backward=False) backward (builder.py:224-233 over e2e_forward), with the aux head where the
    model has one; under torch.autocast(autocast) where given, the loss formed outside it as train.py does.
    Returns feats, low, aux_low and the losses as a namespace."""
    with torch.autocast("cpu", dtype=autocast) if autocast is not None else contextlib.nullcontext():
        feats, low, out = e2e_forward(model, rgb, dep, bases)
        aux_low = model.aux_head(feats[model.aux_index]) if model.aux_head is not None else None
    valid = lab != cfg.background
    loss = loss_main = model.criterion(out.to(rgb.dtype), lab)[valid].mean()
    loss_aux = None
    if aux_low is not None:
        aux = F.interpolate(aux_low, size=rgb.shape[2:], mode="bilinear", align_corners=False)
        loss_aux = model.criterion(aux.to(rgb.dtype), lab)[valid].mean()
        loss = loss_main + model.aux_rate * loss_aux
    if backward:
        loss.backward()
    return types.SimpleNamespace(feats=feats, low=low, aux_low=aux_low, loss_main=loss_main, loss_aux=loss_aux,
                                 loss=loss)
