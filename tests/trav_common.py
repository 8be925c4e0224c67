"""Shared by tests/test_trav_*.py and oracle/golden_e2e.py: deterministic values for the DFormerTrav
keys gen.param_value does not know (query1 / query2 / in_proj_*), the scans, and a torch float64
restatement of what Attention1Dto2D (DFormer.py:308-339) computes once it is collapsed.
Nothing here touches the package under test or the reference."""
import numpy as np
import torch

import gen

EXPAND = "attn_expand_e."


def expand_value(name, shape, wseed, ascale):
    """The value of one Attention1Dto2D key: gen.param_value's rules for the nn.Linear children, N(0, 1)
    queries (query1 scaled by `ascale`, which sets the spread of alpha), U(-1, 1) / sqrt(E) in_proj weights and
    U(-0.1, 0.1) in_proj biases; all drawn from the seed `wseed`."""
    leaf = name.split(".")[-1]
    g = gen.rng(wseed, name)
    shape = tuple(shape)
    if leaf == "query1":
        return g.standard_normal(shape) * ascale
    if leaf == "query2":
        return g.standard_normal(shape)
    if leaf == "in_proj_weight":
        return g.uniform(-1.0, 1.0, shape) / np.sqrt(shape[1])
    if leaf == "in_proj_bias":
        return g.uniform(-0.1, 0.1, shape)
    return gen.param_value(name, shape, wseed)


def state_values(named_shapes, wseed, ascale):
    """{key: ndarray} for a whole state dict: the expansion's keys by expand_value, the rest by gen.param_value
    with its default seed."""
    out = {}
    for k, s in named_shapes:
        if EXPAND in k or k.split(".")[0] in ("query1", "query2", "input_proj", "attn1", "attn2", "output_proj"):
            out[k] = expand_value(k, s, wseed, ascale)
        else:
            out[k] = gen.param_value(k, s)
    return out


def load_values(module, wseed, ascale):
    sd = module.state_dict()
    vals = state_values([(k, v.shape) for k, v in sd.items()], wseed, ascale)
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(sd[k].dtype) for k, v in vals.items()})
    return module


def scans(name, B, N):
    """Laser ranges in metres: U(0.5, 10)."""
    return gen.uniform(name + "/x", (B, N), 0.5, 10.0)


def fold64(p, E=64, Hh=4):
    """(alpha [L, Hh], g [Hh], c []) in float64 from the expansion's parameters p (a dict of tensors under the
    module's own keys): the parameter fold of the collapse."""
    d = torch.float64
    dh = E // Hh
    w_in, b_in = p["input_proj.weight"].to(d)[:, 0], p["input_proj.bias"].to(d)
    w1, b1 = p["attn1.in_proj_weight"].to(d), p["attn1.in_proj_bias"].to(d)
    w2, b2 = p["attn2.in_proj_weight"].to(d), p["attn2.in_proj_bias"].to(d)
    wo1, bo1 = p["attn1.out_proj.weight"].to(d), p["attn1.out_proj.bias"].to(d)
    wo2, bo2 = p["attn2.out_proj.weight"].to(d), p["attn2.out_proj.bias"].to(d)
    w_out, b_out = p["output_proj.weight"].to(d)[0], p["output_proj.bias"].to(d)[0]
    q = p["query1"].to(d) @ w1[:E].t() + b1[:E]
    kw = w1[E:2 * E] @ w_in
    alpha = (q.view(-1, Hh, dh) * kw.view(Hh, dh)).sum(-1) / dh ** 0.5
    u = wo1.t() @ (w2[2 * E:].t() @ (wo2.t() @ w_out))
    g = (u.view(Hh, dh) * (w1[2 * E:] @ w_in).view(Hh, dh)).sum(-1)
    c = u @ (w1[2 * E:] @ b_in + b1[2 * E:]) + w_out @ (wo2 @ (w2[2 * E:] @ bo1 + b2[2 * E:]) + bo2) + b_out
    return alpha, g, c


def collapse64(x, alpha, g, c):
    """s [B, L], mean, var [B, L, Hh] in float64 from scans x [B, N]: the softmax-weighted mean and variance of
    the scan under the logits alpha[l, h] * x[b, j], and s = c + sum_h g[h] * mean."""
    x = x.to(torch.float64)
    w = torch.softmax(alpha[None, :, :, None] * x[:, None, None, :], dim=-1)  # [B, L, Hh, N]
    mean = (w * x[:, None, None, :]).sum(-1)
    var = (w * (x[:, None, None, :] - mean[..., None]) ** 2).sum(-1)
    return c + (mean * g).sum(-1), mean, var


def collapse_grads64(dplane, g, mean, var):
    """(ds, dalpha, dg, dc) in float64 from the upstream gradient of the plane [B, Hout, L]."""
    ds = dplane.to(torch.float64).sum(1)
    return ds, g * (ds[..., None] * var).sum(0), (ds[..., None] * mean).sum((0, 1)), ds.sum()


ZERO_SET = ("query2", "attn2.in_proj_weight[:2E]", "attn2.in_proj_bias[:2E]", "attn1.in_proj_bias[E:2E]")


def zero_parts(grads, E=64):
    """The slices of the expansion's gradients that are exactly zero in the reference."""
    return {"query2": grads["query2"], "attn2.in_proj_weight[:2E]": grads["attn2.in_proj_weight"][:2 * E],
            "attn2.in_proj_bias[:2E]": grads["attn2.in_proj_bias"][:2 * E],
            "attn1.in_proj_bias[E:2E]": grads["attn1.in_proj_bias"][E:2 * E]}
