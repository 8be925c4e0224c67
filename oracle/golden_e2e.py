"""End-to-end fixtures: the reference's EncoderDecoder trained for one step on CPU in float64 (e2e_*), the
reference's own low-precision error on the same step (bf16env_* / fp32env_* / f16env_* files, env/* arrays), the
Trav backbone's laser-scan expansion (trav_expand_*), few-shot episodes (e2e_fss_small) and optimizer groups.

Every step goes through golden_common.train_step: the backbone's `(outs, None)` tuple is indexed before the
decode head and the loss of builder.py:230-232 applied by hand. Inputs are gen.rgb_depth(seed)
and gen.labels; where a fixture searches its input seed, the seed is in meta.
"""
import numpy as np
import torch

import gen
from golden_common import (e2e_forward, e2e_seeds, f32, fp_rel_err, gfp, group_names, gw_names, ham_relus, inject_bases,
                           build_segmentor, load, lowp_env, env_summary, module_relus, ref, rel, relu_margin, save,
                           sd_names, search_seed, t, train_step)


def golden_e2e(name, backbone, B, H, W, decoder="ham", ncls=40, embed=512, backward=True, margin=None, tries=200):
    """End-to-end golden (features, logits, loss, input and parameter gradient fingerprints). With `margin`
    (ham decoder) the input draw is the first seed from 8964 whose decoder ReLU inputs all stay at least
    margin x max away from the kink, so an fp32 run cannot flip an activation against fp64 by summation
    order alone (round 5's e2e_tiny_small had one align-ReLU input at 6e-7 of max: a reduction-geometry
    change flipped it and moved every gradient behind it by up to 1.2e-2); the seed is meta[4]."""
    model, cfg = build_segmentor(backbone, decoder, ncls, embed)
    model.train()
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases") if decoder == "ham" else None
    seed = e2e_seeds(1)[0]
    if margin is not None:
        def margin_of(s):
            rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=s)
            return relu_margin(model, lambda: e2e_forward(model, t(rgb_np, False), t(dep_np, False), bases),
                               ham_relus(model.decode_head))
        seed, mg = search_seed(margin_of, e2e_seeds(tries), margin)
        print(f"  {name}: input seed {seed}, decoder ReLU margin {mg:.2e}")
    rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=seed)
    rgb, dep = t(rgb_np, backward), t(dep_np, backward)
    lab = torch.from_numpy(gen.labels(B, H, W, ncls))
    if not backward:
        with torch.no_grad():
            feats, low, out = e2e_forward(model, rgb, dep, bases)
        save(name, low_fp=gen.fingerprint(low.numpy()), out_fp=gen.fingerprint(out.numpy()),
             **{f"feat{i}_fp": gen.fingerprint(f.numpy()) for i, f in enumerate(feats)},
             meta=np.array([B, H, W, ncls]))
        return
    r = train_step(model, cfg, rgb, dep, lab, bases)
    save(name, low=r.low.detach().numpy().astype(np.float32), loss=np.array(r.loss.item()),
         grgb_fp=gen.fingerprint(rgb.grad.numpy()), gdep_fp=gen.fingerprint(dep.grad.numpy()),
         **{f"feat{i}": f.detach().numpy().astype(np.float32) for i, f in enumerate(r.feats)},
         meta=np.array([B, H, W, ncls] + ([seed] if margin is not None else [])), **gfp(model))


def golden_e2e_env(prefix, dtype, name, backbone, B, H, W, decoder="ham", ncls=40, embed=512):
    """<prefix><name>.npz: the reference's OWN error on the e2e golden `name`: the same model, weights and inputs
    in float32 (dtype None), or in float32 under torch.autocast(dtype) on CPU (what train.py's --amp does),
    compared with the fp64 golden. The HIP paths are gated against these envelopes (reference bf16
    autocast misses a plain 1e-2 end-to-end gate by itself)."""
    g = load(name)
    dtype = getattr(torch, dtype) if dtype else None  # the registry names it
    model, cfg = build_segmentor(backbone, decoder, ncls, embed, dtype=torch.float32)
    model.train()
    rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=int(g["meta"][4]) if g["meta"].size > 4 else e2e_seeds(1)[0])
    rgb, dep = f32(rgb_np).requires_grad_(), f32(dep_np).requires_grad_()
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases") if decoder == "ham" else None
    r = train_step(model, cfg, rgb, dep, torch.from_numpy(gen.labels(B, H, W, ncls)), bases, autocast=dtype)
    env = lowp_env(g, dict(low=r.low, loss=r.loss.item()))
    env["env/grgb"] = np.array(fp_rel_err(gen.fingerprint(rgb.grad.double().numpy()), g["grgb_fp"]))
    env.update(lowp_env(g, {}, model))
    print(f"  {prefix} envelope {name}: {env_summary(env)}")
    save(prefix + name, **env)


def _with_env(arrays, golden, low, m32):
    """arrays + the reference's own float32 error of the same step (golden_e2e_env with dtype None)."""
    env = lowp_env({**arrays, **golden}, low, m32)
    print(f"    fp32 envelope {env_summary(env)}")
    arrays.update(env)
    return arrays


def golden_e2e_aux(name, ncls, base="e2e_tiny_small", margin=3e-6):
    """DFormer-Tiny + ham with aux_rate = 0.4 (builder.py:138-143, 204-207, 231-232) on the inputs of `base`
    (its shape, input seed meta[4] and bases). builder.py:143 binds cfg.num_classes to FCNHead's hidden width and
    leaves its num_classes at 40, so aux_low is [B, 40, H/16, W/16] for 37 classes too. With 40 classes the main
    path is base's: `low` and the main loss are asserted equal to it. Stored: aux_low, loss_main, loss_aux, loss,
    gfp/<key>, auxgrad/<key> (the aux head's gradients in full), env/..., margin (the aux ReLU's), sd_keys /
    sd_shapes, gw_decay / gw_nodecay, meta = [B, H, W, ncls, seed]."""
    g0 = load(base)
    B, H, W = [int(v) for v in g0["meta"][:3]]
    seed = int(g0["meta"][4])
    rgb_np, dep_np = gen.rgb_depth(B, H, W, seed=seed)
    lab = torch.from_numpy(gen.labels(B, H, W, ncls)).long()
    bases = gen.nmf_bases(B, 512, 64, name=base + "/bases")
    model, cfg = build_segmentor("DFormer-Tiny", ncls=ncls, aux_rate=0.4)
    model.train()
    rgb, dep = t(rgb_np, False), t(dep_np, False)
    mg = relu_margin(model, lambda: train_step(model, cfg, rgb, dep, lab, bases, backward=False),
                     module_relus(model.aux_head))
    assert mg > margin, f"aux ReLU margin {mg:.3e} <= {margin}"
    r = train_step(model, cfg, rgb, dep, lab, bases)
    assert tuple(r.aux_low.shape) == (B, 40, H // 16, W // 16), r.aux_low.shape
    print(f"  {name}: aux ReLU margin {mg:.2e}, main loss {r.loss_main.item():.6f}, aux loss {r.loss_aux.item():.6f}")
    if ncls == int(g0["meta"][3]):  # the main path is the existing golden's
        dlow = np.abs(r.low.detach().numpy() - g0["low"].astype(np.float64)).max()
        assert dlow < 2e-7 * max(np.abs(g0["low"]).max(), 1.0), dlow
        assert abs(r.loss_main.item() - float(g0["loss"])) < 1e-12 * abs(float(g0["loss"])) + 1e-15
    arrays = gfp(model)
    for n, p in model.aux_head.named_parameters():
        arrays["auxgrad/aux_head." + n] = p.grad.numpy().astype(np.float32)
    arrays.update(sd_names(model), **gw_names(model))
    m32, _ = build_segmentor("DFormer-Tiny", ncls=ncls, aux_rate=0.4, dtype=torch.float32)
    r32 = train_step(m32.train(), cfg, f32(rgb_np), f32(dep_np), lab, bases)
    golden = dict(aux_low=r.aux_low, loss=r.loss.item())
    _with_env(arrays, golden, dict(aux_low=r32.aux_low, loss=r32.loss.item()), m32)
    save(name, aux_low=r.aux_low.detach().numpy().astype(np.float32), loss_main=np.array(r.loss_main.item()),
         loss_aux=np.array(r.loss_aux.item()), loss=np.array(r.loss.item()), margin=np.array(mg),
         meta=np.array([B, H, W, ncls, seed]), **arrays)


def golden_e2e_uper(name, B=2, H=64, W=96, ncls=40, tries=200):
    """DFormer-Tiny + UPernet with its hard-coded aux head (builder.py:145-152, 204-207, 231-232) on the
    e2e_tiny_small recipe. At 512 channels the head has ~1.5 M ReLU inputs and no seed keeps them all off the kink:
    the best seed of `tries` is taken and its margin recorded; gradients are gated through env/. Stored: low,
    aux_low, loss_main, loss_aux, loss, gfp/<key>, env/..., sd_keys / sd_shapes, gw_decay / gw_nodecay, margin,
    meta = [B, H, W, ncls, seed]."""
    model, cfg = build_segmentor("DFormer-Tiny", "UPernet", ncls)
    model.train()
    assert model.aux_rate == 0.4 and model.aux_index == 2  # builder.py:150-151
    lab = torch.from_numpy(gen.labels(B, H, W, ncls)).long()
    inputs = lambda s, cast: [cast(a) for a in gen.rgb_depth(B, H, W, seed=s)]  # noqa: E731
    seed, mg = search_seed(lambda s: relu_margin(model, lambda: e2e_forward(model, *inputs(s, lambda a: t(a, False))),
                                                 module_relus(model.decode_head)), e2e_seeds(tries))
    print(f"  {name}: best of {tries} seeds: {seed}, decode-head ReLU margin {mg:.2e}")
    r = train_step(model, cfg, *inputs(seed, lambda a: t(a, False)), lab)
    assert tuple(r.low.shape) == (B, ncls, H // 4, W // 4), r.low.shape
    arrays = {**gfp(model), **sd_names(model), **gw_names(model)}
    m32, _ = build_segmentor("DFormer-Tiny", "UPernet", ncls, dtype=torch.float32)
    r32 = train_step(m32.train(), cfg, *inputs(seed, f32), lab)
    _with_env(arrays, dict(low=r.low, aux_low=r.aux_low, loss=r.loss.item()),
              dict(low=r32.low, aux_low=r32.aux_low, loss=r32.loss.item()), m32)
    save(name, low=r.low.detach().numpy().astype(np.float32), aux_low=r.aux_low.detach().numpy().astype(np.float32),
         loss_main=np.array(r.loss_main.item()), loss_aux=np.array(r.loss_aux.item()), loss=np.array(r.loss.item()),
         margin=np.array(mg), meta=np.array([B, H, W, ncls, seed]), **arrays)


# ------------------------------------------------------------------------------- DFormerTrav
def _assert_zero_set(grads):
    """query2 and attn2's Q / K thirds sit behind a softmax over one key, whose backward is p * (1 - p) = 0
    exactly. The K third of attn1.in_proj_bias shifts every logit of a softmax row alike: its gradient is
    mathematically zero, and the reference leaves rounding noise there (about 1e-17 of the bias gradient)."""
    import trav_common as TC
    for k, v in TC.zero_parts(grads).items():
        if k.startswith("attn1."):
            noise = (v.abs().max() / grads["attn1.in_proj_bias"].abs().max()).item()
            assert noise < 1e-12, f"{k}: {noise:.2e} of the bias gradient"
        else:
            assert torch.count_nonzero(v) == 0, f"{k}: the reference's gradient is not exactly zero"


def _search_weights(N, L, Hout, x, tries=40):
    """(module, wseed, ascale, cond) of the first trav_common weight draw for Attention1Dto2D(N, L, Hout) whose
    cond = [max|alpha| * std(x), min_h|g| / max_h|g|] has cond[0] in [3, 12] and cond[1] >= 0.05, so that the
    queries matter, the softmax is neither flat nor one-hot and every head reaches the output (at a default init
    a wrong head or query mapping would be invisible): seeds from 1234 (for g), ascale over a geometric grid."""
    import trav_common as TC
    for wseed in range(1234, 1234 + tries):
        for ascale in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0):
            mod = TC.load_values(ref().dformer.Attention1Dto2D(N, L, Hout, 64, 4), wseed, ascale)
            alpha, g, _ = TC.fold64({k: v.detach() for k, v in mod.state_dict().items()})
            cond = np.array([alpha.abs().max().item() * float(np.std(x)), (g.abs().min() / g.abs().max()).item()])
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
    """The reference's Attention1Dto2D (models/encoders/DFormer.py:308-339) alone on trav_common.scans(name),
    upstream gradient gen.normal(name + "/gy") on the plane. The plane is asserted constant along H; stored are its
    one distinct row `s` [B, L], every parameter gradient in full, env/s and env/grad/<key> (the module itself in
    float32), wmeta = [wseed, ascale], cond, meta = [B, N, L, Hout]. The zero set is asserted (_assert_zero_set)."""
    import trav_common as TC
    x = TC.scans(name, B, N)
    mod, wseed, ascale, cond = _search_weights(N, L, Hout, x)
    print(f"  {name}: wseed {wseed} ascale {ascale} max|alpha|*std(x) {cond[0]:.2f} min|g|/max|g| {cond[1]:.3f}")
    gy = gen.normal(name + "/gy", (B, 1, Hout, L))
    plane, grads = _expand_step(mod, x, gy, torch.float64)
    assert tuple(plane.shape) == (B, 1, Hout, L)
    assert torch.equal(plane, plane[:, :, :1].expand_as(plane)), "the plane is not constant along H"
    s = plane[:, 0, 0]
    _assert_zero_set(grads)
    s_c, _, _ = TC.collapse64(torch.from_numpy(x), *TC.fold64(mod.state_dict()))
    print(f"  {name}: collapse formula vs module {rel(s_c.numpy(), s.numpy()):.2e} at scale {s.abs().max().item():.1f}")
    m32 = TC.load_values(ref().dformer.Attention1Dto2D(N, L, Hout, 64, 4), wseed, ascale)
    p32, g32 = _expand_step(m32, x, gy, torch.float32)
    arrays = {"grad/" + n: v.numpy().astype(np.float32) for n, v in grads.items()}
    arrays.update(lowp_env(dict(s=s), dict(s=p32[:, 0, 0])))
    arrays.update(lowp_env(grads, {n: g32[n] for n, v in grads.items() if torch.count_nonzero(v) > 0}, prefix="env/grad/"))
    save(name, s=s.numpy(), meta=np.array([B, N, L, Hout]), wmeta=np.array([wseed, ascale], np.float64),
         cond=cond, **arrays)


def golden_e2e_trav(name, B=2, H=64, W=96, N=24, ncls=2, margin=3e-6, tries=100):
    """EncoderDecoder(backbone="DFormerTrav-Base", decoder="ham") (models/builder.py:109-111) with attn_expand_e at
    (N, W, H), RGB B x 3 x H x W, scans and weights from trav_common. Stored: low, loss, gfp/<key>, sd_keys /
    sd_shapes, gw_decay / gw_nodecay, env/low, env/loss, env/gfp/<key>, margin (the decoder ReLUs'), wmeta, cond,
    meta = [B, H, W, ncls, input seed, N]."""
    import trav_common as TC
    x = TC.scans(name, B, N)
    _, wseed, ascale, cond = _search_weights(N, W, H, x)
    print(f"  {name}: wseed {wseed} ascale {ascale} cond {cond}")
    build = lambda dtype: build_segmentor("DFormerTrav-Base", ncls=ncls, expand=(N, W, H), values=(wseed, ascale),  # noqa: E731
                                          dtype=dtype)
    model, cfg = build(torch.float64)
    model.train()
    bases = gen.nmf_bases(B, 512, 64, name=name + "/bases")
    scan = torch.from_numpy(x).unsqueeze(1)
    rgb_of = lambda s: gen.rgb_depth(B, H, W, seed=s)[0]  # noqa: E731
    seed, mg = search_seed(lambda s: relu_margin(model, lambda: e2e_forward(model, t(rgb_of(s), False), scan, bases),
                                                 ham_relus(model.decode_head)), e2e_seeds(tries), margin)
    print(f"  {name}: input seed {seed}, decoder ReLU margin {mg:.2e}")
    lab = torch.from_numpy(gen.labels(B, H, W, ncls)).long()
    r = train_step(model, cfg, t(rgb_of(seed), False), scan, lab, bases)
    arrays = gfp(model)
    _assert_zero_set({n[len("encoder_backbone.attn_expand_e."):]: p.grad for n, p in model.named_parameters()
                      if ".attn_expand_e." in n})
    arrays.update(sd_names(model), **gw_names(model))
    m32 = build(torch.float32)[0].train()
    r32 = train_step(m32, cfg, f32(rgb_of(seed)), scan.float(), lab, bases)
    _with_env(arrays, dict(low=r.low, loss=r.loss.item()), dict(low=r32.low, loss=r32.loss.item()), m32)
    save(name, low=r.low.detach().numpy().astype(np.float32), loss=np.array(r.loss.item()), margin=np.array(mg),
         cond=cond, wmeta=np.array([wseed, ascale], np.float64), meta=np.array([B, H, W, ncls, seed, N]), **arrays)


# ------------------------------------------------------------------------------- few-shot episodes
FSS = "e2e_fss_small"
LOSS_GATE = 1e-4


def _episode(model, inp, bases, q_gt=None, swap=False):
    """The reference's meta_forward with the injected bases; records what `similarity` receives and returns and
    the decode head's logits. swap: the two prototypes exchanged (the generator's sensitivity condition)."""
    import fss_common as FC
    inject_bases(model, bases, inp["q_rgb"].dtype)
    seen = {"proto": [], "sim": []}
    orig = model.similarity
    calls = []

    def similarity(feat, proto, scaler=20):
        calls.append(proto)
        out = orig(feat, proto, scaler)
        seen["proto"].append(proto.detach().reshape(-1))
        seen["sim"].append(out.detach())
        return out

    def swapped(feat, proto, scaler=20):  # fg_sim is asked for first (builder.py:294-295): hand out the other one
        i = len(calls)
        calls.append(proto)
        return orig(feat, swapped.other[i], scaler)

    head_forward = model.decode_head.forward  # decode() calls .forward itself: a module hook would not fire

    def forward(feats):
        out = head_forward(feats)
        seen["low"] = out.detach()
        return out

    model_encode = model.encode

    def encode(rgb, modal_x):
        feats = model_encode(rgb, modal_x)
        seen["f3"] = feats[-1].detach()
        return feats

    model.decode_head.forward = forward
    model.encode = encode
    model.similarity = similarity
    try:
        if swap:
            with torch.no_grad():
                model.meta_forward(inp["s_rgb"], inp["s_depth"], inp["s_mask"], inp["q_rgb"], inp["q_depth"], q_gt)
            protos = list(calls)
            swapped.other = [protos[i ^ 1] for i in range(len(protos))]
            calls.clear()
            model.similarity = swapped
        out = model.meta_forward(inp["s_rgb"], inp["s_depth"], inp["s_mask"], inp["q_rgb"], inp["q_depth"], q_gt)
    finally:
        del model.similarity
        del model.encode
        del model.decode_head.forward
    if not swap:
        B = inp["q_rgb"].shape[0]
        fg, bg = seen["proto"][0::2], seen["proto"][1::2]  # per query image: fg first, then bg
        seen["proto"] = torch.stack([torch.stack([bg[b], fg[b]]) for b in range(B)])
        sims = torch.stack([torch.stack([seen["sim"][2 * b + 1][0], seen["sim"][2 * b][0]], -1) for b in range(B)])
        seen["prob"] = torch.softmax(sims / FC.E2E["temperature"], -1)  # [B, hs, ws, 2]
    return out, seen


def _fss_inputs(seed, mseed, dtype=torch.float64, empty=()):
    import fss_common as FC
    import trav_common as TC
    B, S, H, W, N = (FC.E2E[k] for k in ("B", "S", "H", "W", "N"))
    rgb, _ = gen.rgb_depth(B * S + B, H, W, seed=seed)
    x = TC.scans(FSS, B * S + B, N)
    m = FC.masks(FSS, B * S, H, W, seed=mseed, empty=empty)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    return dict(s_rgb=tt(rgb[:B * S]).view(B, S, 3, H, W), q_rgb=tt(rgb[B * S:]),
                s_depth=tt(x[:B * S]).view(B, S, 1, N), q_depth=tt(x[B * S:]).view(B, 1, N),
                s_mask=torch.from_numpy(m).view(B, S, H, W))


def golden_fss(margin=1e-6, tries=300):
    """e2e_fss_small: the reference's EncoderDecoder.meta_forward (models/builder.py:237-320) with the Trav
    backbone + ham at fss_common.E2E (B episodes of S shots, attn_expand_e at (N, W, H), alpha, temperature),
    injected NMF bases (one set per image of the query batch). Stored: proto [B, 2, C] (row 0 = bg, 1 = fg: what
    the reference passes to `similarity`), prob (softmax over [bg, fg] of its similarities / temperature), low
    (the decode head's logits; low64 in float64), f3 (the stage-3 map of the B*S + B images, float64: the input of
    the CPU restatement), loss, gfp/<key>, fused_eval (the fused logits of an eval-mode call on the same weights),
    env/<name> (the reference's own float32 error of each; env/gfp is one array aligned with gfp_keys), margin,
    proto_empty / prob_empty / loss_empty (the same training forward with support image 1 stripped of its
    foreground), cond, wmeta, meta = [B, S, H, W, N, input seed, mask seed].
    The seeds are searched until the conditions hold: prob[..., 1] has standard deviation >= 0.05 over the cells
    and lies inside (0.02, 0.98) on at least half of them; the loss recomputed with the two prototypes swapped
    moves by more than 100 x the loss gate (1e-4 relative); every support image has both classes.
    margin: e2e_trav_small asks 3e-6 of its 64 x 96 images; the 96 x 128 queries here put about 8e5 values
    through the head's ReLUs, whose smallest |input| / max |input| is then of the order of 1e-6 itself."""
    import fss_common as FC
    import trav_common as TC
    E = FC.E2E
    B, S, H, W, N = (E[k] for k in ("B", "S", "H", "W", "N"))
    _, wseed, ascale, _ = _search_weights(N, W, H, TC.scans(FSS, B * S + B, N))
    build = lambda dtype: build_segmentor("DFormerTrav-Base", ncls=E["ncls"], expand=(N, W, H), dtype=dtype,  # noqa: E731
                                          values=(wseed, ascale), alpha=E["alpha"], temperature=E["temperature"])[0]
    model = build(torch.float64).train()
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    bases = gen.nmf_bases(B, 512, 64, name=FSS + "/bases")
    lab = torch.from_numpy(FC.masks(FSS + "/q", B, H, W))
    holds = lambda c: c[0] >= 0.05 and c[1] >= 0.5 and c[2] > 100 * LOSS_GATE  # noqa: E731
    for k, seed in enumerate(e2e_seeds(tries)):
        mseed = 77 + k
        inp = _fss_inputs(seed, mseed)
        sm = inp["s_mask"].view(B * S, H, W)
        if not all(((sm[i] == 0).any() and (sm[i] == 1).any()) for i in range(B * S)):
            continue
        mg = relu_margin(model, lambda: _episode(model, inp, bases), ham_relus(model.decode_head))
        if mg <= margin:
            print(f"  {FSS}: seed {seed} margin {mg:.2e}: too close to a ReLU kink")
            continue
        with torch.no_grad():
            (loss, _), seen = _episode(model, inp, bases, lab)
            model.load_state_dict(sd0)
            (loss_sw, _), _ = _episode(model, inp, bases, lab, swap=True)
            model.load_state_dict(sd0)
        fg = seen["prob"][..., 1].reshape(-1)
        cond = np.array([fg.std().item(), ((fg > 0.02) & (fg < 0.98)).double().mean().item(),
                         abs(loss_sw.item() - loss.item()) / abs(loss.item())])
        print(f"  {FSS}: seed {seed} margin {mg:.2e} prob std {cond[0]:.3f} inside {cond[1]:.2f} swap {cond[2]:.2e}")
        if holds(cond):
            break
    else:
        raise RuntimeError("no seed meets the conditions")

    def step(m, inp_, b):
        (loss_, _), seen_ = _episode(m, inp_, b, lab)
        loss_.backward()
        return loss_.item(), seen_

    loss, seen = step(model, inp, bases)
    arrays = gfp(model)
    model.load_state_dict(sd0)
    model.eval()
    with torch.no_grad():
        fused_eval, _ = _episode(model, inp, bases)
    model.train()
    model.load_state_dict(sd0)
    inp_e = _fss_inputs(seed, mseed, empty=(1,))
    assert not (inp_e["s_mask"].view(B * S, H, W)[1] == 1).any()
    with torch.no_grad():
        (loss_e, _), seen_e = _episode(model, inp_e, bases, lab)
    # the reference's own float32 error
    m32 = build(torch.float32).train()
    inp32 = _fss_inputs(seed, mseed, torch.float32)
    loss32, seen32 = step(m32, inp32, bases)
    # one array for the fingerprints' envelopes, aligned with gfp_keys: a second entry per parameter would
    # take the file past the size a committed fixture may have
    genv = lowp_env(arrays, {}, m32, prefix="")
    assert len(genv) == len(arrays)
    arrays["gfp_keys"] = np.array([k[len("gfp/"):] for k in genv])
    arrays["env/gfp"] = np.array([float(v) for v in genv.values()])
    with torch.no_grad():
        fused32, _ = _episode(build(torch.float32).eval(), inp32, bases)
    golden = dict(proto=seen["proto"], prob=seen["prob"], low=seen["low"], loss=loss, fused_eval=fused_eval)
    env = lowp_env(golden, dict(proto=seen32["proto"], prob=seen32["prob"], low=seen32["low"], loss=loss32,
                                fused_eval=fused32))
    print(f"  {FSS}: loss {loss:.6f}; fp32 envelope {env_summary({**env, **{'env/gfp/' + k: v for k, v in genv.items()}})}")
    save(FSS, proto=seen["proto"].numpy(), prob=seen["prob"].numpy(), low=seen["low"].numpy().astype(np.float32),
         loss=np.array(loss), f3=seen["f3"].numpy(), low64=seen["low"].numpy(),
         fused_eval=fused_eval.numpy().astype(np.float32), margin=np.array(mg), cond=cond,
         proto_empty=seen_e["proto"].numpy(), prob_empty=seen_e["prob"].numpy(), loss_empty=np.array(loss_e.item()),
         wmeta=np.array([wseed, ascale], np.float64), meta=np.array([B, S, H, W, N, seed, mseed]), **arrays, **env)


# ------------------------------------------------------------------------------- optimizer groups
def golden_groups():
    """groups_base: optimizer-group membership of group_weight (init_func.py:26-70) for Base + ham, sorted."""
    model, _ = build_segmentor("DFormer-Base")
    decay, nodecay = (sorted(names) for names in group_names(model))
    excluded = sorted({n for n, _ in model.named_parameters()} - set(decay) - set(nodecay))
    save("groups_base", decay=np.array(decay), nodecay=np.array(nodecay), excluded=np.array(excluded),
         counts=np.array([sum(p.numel() for n, p in model.named_parameters() if n in excluded),
                          sum(p.numel() for p in model.parameters())]))
