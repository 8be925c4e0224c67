"""Generate tests/golden/trav_expand_*.npz and e2e_trav_small.npz: the reference's Attention1Dto2D
(models/encoders/DFormer.py:308-339) alone, and EncoderDecoder with backbone "DFormerTrav-Base"
(models/builder.py:109-111) + ham, on CPU in float64.

TEST INFRASTRUCTURE. Run in the build container only (it needs the read-only reference that
oracle/ref_import.py imports):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_trav_goldens.py [name prefix ...]
Nothing under oracle/ changes and nothing of the reference is copied: the files hold arrays and name
lists only. Weights and scans come from tests/trav_common.py (gen.py's seeded draws plus values for the
keys gen.param_value does not know).

trav_expand_small (N=12, L=10, Hout=6, B=3), trav_expand_full (360 / 640 / 480, B=2): the module in
float64 on trav_common.scans(name), upstream gradient gen.normal(name + "/gy") on the plane. The generator
asserts that the plane is constant along H and stores its one distinct row `s` [B, L], every parameter
gradient in full (grad/<key>), env/s and env/grad/<key> (the rel-to-max error of the reference module itself
in float32 on the same inputs), and wmeta = [wseed, ascale]: the weight seed and the query1 scale, searched
until cond = [max|alpha| * std(x), min_h|g| / max_h|g|] has cond[0] in [1, 20] and cond[1] >= 0.05, so that
the queries matter, the softmax is neither flat nor one-hot and every head reaches the output (at a default
init a wrong head or query mapping would be invisible). meta = [B, N, L, Hout]. The zero set is asserted:
query2 and the Q / K thirds of attn2.in_proj_* exactly zero, the K third of attn1.in_proj_bias
(mathematically zero) below 1e-12 of the bias gradient, where the reference leaves rounding noise.

e2e_trav_small: EncoderDecoder(backbone="DFormerTrav-Base", decoder="ham", num_classes=2, aux_rate=0) with
attn_expand_e replaced by the reference's own class at (24, 96, 64), RGB 2 x 3 x 64 x 96, drop_path_rate 0,
injected NMF bases "e2e_trav_small/bases". Stored: low, loss, gfp/<key> (16-sample fingerprints of every
parameter gradient), sd_keys / sd_shapes, gw_decay / gw_nodecay (utils/init_func.py group_weight's two lists
by name), env/low, env/loss, env/gfp/<key> (the reference's own float32 error), margin (the decoder ReLUs'),
wmeta, cond, meta = [B, H, W, ncls, input seed, N].
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen  # noqa: E402
import make_goldens as MG  # noqa: E402  (sets the default dtype to float64 and imports the reference)
import trav_common as TC  # noqa: E402


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _assert_zero_set(grads):
    """query2 and attn2's Q / K thirds sit behind a softmax over one key, whose backward is p * (1 - p) = 0
    exactly. The K third of attn1.in_proj_bias shifts every logit of a softmax row alike: its gradient is
    mathematically zero, and the reference leaves rounding noise there (about 1e-17 of the bias gradient)."""
    for k, v in TC.zero_parts(grads).items():
        if k.startswith("attn1."):
            noise = (v.abs().max() / grads["attn1.in_proj_bias"].abs().max()).item()
            assert noise < 1e-12, f"{k}: {noise:.2e} of the bias gradient"
        else:
            assert torch.count_nonzero(v) == 0, f"{k}: the reference's gradient is not exactly zero"


def _conditions(mod, x):
    alpha, g, _ = TC.fold64({k: v.detach() for k, v in mod.state_dict().items()})
    return np.array([alpha.abs().max().item() * float(np.std(x)), (g.abs().min() / g.abs().max()).item()])


def _search_weights(make, x, tries=40):
    """The first (wseed, ascale) whose conditions hold: seeds from 1234 (for g), ascale over a geometric
    grid aiming at max|alpha| * std(x) near 6."""
    for wseed in range(1234, 1234 + tries):
        for ascale in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0):
            mod = TC.load_values(make(), wseed, ascale)
            cond = _conditions(mod, x)
            if cond[1] < 0.05:
                break  # g does not depend on ascale: next seed
            if 3.0 <= cond[0] <= 12.0:
                return mod, wseed, ascale, cond
    raise RuntimeError("no weight draw meets the alpha / g conditions")


def _expand_step(mod, x, gy, dtype):
    mod = mod.to(dtype)
    plane = mod(torch.from_numpy(x).to(dtype).unsqueeze(1))
    (plane * torch.from_numpy(gy).to(dtype)).sum().backward()
    return plane.detach(), {n: p.grad.detach() for n, p in mod.named_parameters()}


def golden_expand(name, B, N, L, Hout):
    t0 = time.time()
    x = TC.scans(name, B, N)
    make = lambda: MG.dformer.Attention1Dto2D(N, L, Hout, 64, 4)  # noqa: E731
    mod, wseed, ascale, cond = _search_weights(make, x)
    assert 1.0 <= cond[0] <= 20.0 and cond[1] >= 0.05, cond
    print(f"  {name}: wseed {wseed} ascale {ascale} max|alpha|*std(x) {cond[0]:.2f} min|g|/max|g| {cond[1]:.3f}")
    gy = gen.normal(name + "/gy", (B, 1, Hout, L))
    plane, grads = _expand_step(mod, x, gy, torch.float64)
    assert tuple(plane.shape) == (B, 1, Hout, L)
    assert torch.equal(plane, plane[:, :, :1].expand_as(plane)), "the plane is not constant along H"
    s = plane[:, 0, 0]
    _assert_zero_set(grads)
    s_c, mean, var = TC.collapse64(torch.from_numpy(x), *TC.fold64(mod.state_dict()))
    print(f"  {name}: collapse formula vs module {_rel(s_c.numpy(), s.numpy()):.2e} at scale {s.abs().max().item():.1f}")
    m32 = TC.load_values(make(), wseed, ascale)
    p32, g32 = _expand_step(m32, x, gy, torch.float32)
    arrays = {"grad/" + n: v.numpy().astype(np.float32) for n, v in grads.items()}
    arrays["env/s"] = np.array(_rel(p32[:, 0, 0].double().numpy(), s.numpy()))
    for n, v in grads.items():
        if torch.count_nonzero(v) > 0:
            arrays["env/grad/" + n] = np.array(_rel(g32[n].double().numpy(), v.numpy()))
    ev = np.array([v for k, v in arrays.items() if k.startswith("env/grad/")])
    print(f"  {name}: fp32 envelope s {float(arrays['env/s']):.3e} grads median {np.median(ev):.3e} max {ev.max():.3e}")
    MG.save(name, s=s.numpy(), meta=np.array([B, N, L, Hout]), wmeta=np.array([wseed, ascale], np.float64),
            cond=cond, **arrays)
    print(f"  {name}: {time.time() - t0:.1f}s")


# ------------------------------------------------------------------------------------------ end to end
E2E = dict(B=2, H=64, W=96, N=24, ncls=2)


def _build_trav(wseed, ascale, dtype=torch.float64):
    cfg = MG.Cfg(backbone="DFormerTrav-Base", decoder="ham", decoder_embed_dim=512, num_classes=E2E["ncls"],
                 drop_path_rate=0.0, aux_rate=0, device="cpu", pretrained_model=None, bn_eps=1e-3,
                 bn_momentum=0.1, background=255)
    crit = nn.CrossEntropyLoss(reduction="none", ignore_index=255)
    model = MG.builder.EncoderDecoder(cfg=cfg, criterion=crit, norm_layer=nn.BatchNorm2d, syncbn=False)
    model.decode_head.dropout = None
    model.encoder_backbone.attn_expand_e = MG.dformer.Attention1Dto2D(E2E["N"], E2E["W"], E2E["H"], 64, 4)
    TC.load_values(model, wseed, ascale)
    return model.to(dtype).train(), cfg


def _trav_forward(model, rgb, scan, bases):
    """builder.py:193-208 with the injected NMF bases (the Trav backbone returns the list itself)."""
    model.decode_head.hamburger.ham._build_bases = \
        lambda B_, S, D, R, cuda=False: torch.from_numpy(bases.copy()).to(rgb.dtype)
    feats = model.encoder_backbone(rgb, scan)
    assert isinstance(feats, list) and len(feats) == 4
    low = model.decode_head.forward(feats)
    return low, F.interpolate(low, size=rgb.shape[-2:], mode="bilinear", align_corners=False)


def _relu_margin(model, rgb, scan, bases):
    """min |input| / max |input| over the ham head's ReLUs (as make_goldens._e2e_relu_margin)."""
    head = model.decode_head
    seen = {}
    hooks = [head.squeeze.activate.register_forward_pre_hook(lambda m, a: seen.__setitem__("squeeze", a[0].clone())),
             head.align.activate.register_forward_pre_hook(lambda m, a: seen.__setitem__("align", a[0].clone())),
             head.hamburger.ham_in.register_forward_hook(lambda m, a, o: seen.__setitem__("ham_in", o.clone())),
             head.hamburger.register_forward_pre_hook(lambda m, a: seen.__setitem__("x", a[0].clone())),
             head.hamburger.ham_out.register_forward_hook(lambda m, a, o: seen.__setitem__("ham_out", o.clone()))]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        _trav_forward(model, rgb, scan, bases)
    model.load_state_dict(sd)
    for h in hooks:
        h.remove()
    seen["ham"] = seen.pop("x") + seen.pop("ham_out")
    return min((v.abs().min() / v.abs().max()).item() for v in seen.values())


def golden_e2e_trav(name, margin=3e-6, tries=100):
    t0 = time.time()
    B, H, W, N, ncls = (E2E[k] for k in ("B", "H", "W", "N", "ncls"))
    x = TC.scans(name, B, N)
    _, wseed, ascale, cond = _search_weights(lambda: MG.dformer.Attention1Dto2D(N, W, H, 64, 4), x)
    print(f"  {name}: wseed {wseed} ascale {ascale} cond {cond}")
    model, cfg = _build_trav(wseed, ascale)
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases")
    scan = torch.from_numpy(x).unsqueeze(1)
    for seed in range(8964, 8964 + tries):
        rgb_np, _ = gen.rgb_depth(B, H, W, seed=seed)
        mg = _relu_margin(model, MG.t(rgb_np, False), scan, bases)
        if mg > margin:
            break
    else:
        raise RuntimeError(f"no input seed with ReLU margin > {margin}")
    print(f"  {name}: input seed {seed}, decoder ReLU margin {mg:.2e}")
    lab = torch.from_numpy(gen.labels(B, H, W, ncls)).long()

    def step(m, rgb, sc, b):
        low, out = _trav_forward(m, rgb, sc, b)
        loss = m.criterion(out, lab)[lab != cfg.background].mean()
        loss.backward()
        return low.detach(), loss.item()

    low, loss = step(model, MG.t(rgb_np, False), scan, bases)
    arrays = {"gfp/" + n: gen.fingerprint(p.grad.numpy(), 16) for n, p in model.named_parameters()
              if p.grad is not None}
    ex = {n[len("encoder_backbone.attn_expand_e."):]: p.grad for n, p in model.named_parameters()
          if ".attn_expand_e." in n}
    _assert_zero_set(ex)
    sd = model.state_dict()
    arrays["sd_keys"] = np.array(list(sd.keys()))
    arrays["sd_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    from utils.init_func import group_weight  # noqa: E402  (the reference, read-only)
    groups = group_weight([], model, nn.BatchNorm2d, 6e-5)
    ids = {id(p): n for n, p in model.named_parameters()}
    arrays["gw_decay"] = np.array([ids[id(p)] for p in groups[0]["params"]])
    arrays["gw_nodecay"] = np.array([ids[id(p)] for p in groups[1]["params"]])
    m32, _ = _build_trav(wseed, ascale, torch.float32)
    low32, loss32 = step(m32, torch.from_numpy(rgb_np).float(), scan.float(), bases.astype(np.float32))
    arrays["env/low"] = np.array(_rel(low32.double().numpy(), low.numpy()))
    arrays["env/loss"] = np.array(abs(loss32 - loss) / abs(loss))
    for n, p in m32.named_parameters():
        if p.grad is not None and "gfp/" + n in arrays:
            arrays["env/gfp/" + n] = np.array(MG._fp_rel_err(gen.fingerprint(p.grad.double().numpy(), 16),
                                                             arrays["gfp/" + n], atol=1e-4))
    gv = np.array([v for k, v in arrays.items() if k.startswith("env/gfp/")])
    print(f"  {name}: loss {loss:.6f}; fp32 envelope low {float(arrays['env/low']):.3e} loss "
          f"{float(arrays['env/loss']):.3e} param-grad median {np.median(gv):.3e} max {gv.max():.3e}")
    MG.save(name, low=low.numpy().astype(np.float32), loss=np.array(loss), margin=np.array(mg), cond=cond,
            wmeta=np.array([wseed, ascale], np.float64), meta=np.array([B, H, W, ncls, seed, N]), **arrays)
    print(f"  {name}: {time.time() - t0:.1f}s")


def main():
    which = sys.argv[1:]
    torch.manual_seed(0)

    def want(n):
        return not which or any(n.startswith(w) for w in which)

    if want("trav_expand_small"):
        golden_expand("trav_expand_small", 3, 12, 10, 6)
    if want("trav_expand_full"):
        golden_expand("trav_expand_full", 2, 360, 640, 480)
    if want("e2e_trav_small"):
        golden_e2e_trav("e2e_trav_small")


if __name__ == "__main__":
    main()
