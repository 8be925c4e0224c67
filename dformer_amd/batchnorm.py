"""BatchNorm / SyncBatchNorm on NHWC rows [B*h*w, C], shared by the backbone's stems and every decoder
head: the statistics, the SyncBN collectives and the one forward / backward every conv + BN function uses.

Train mode normalises with batch statistics and updates the running ones like torch; with a multi-rank
process group and SyncBN, the (sum, sumsq) and the backward (sum dy, sum dy*xhat) statistics are
all-reduced (SyncBatchNorm semantics). Eval mode normalises with the running statistics, where BN is a
fixed per-channel affine, in the backward too.
"""
import torch
import torch.distributed as dist

from . import kernels as K
from .functional import gslot_rows


# Test-only: with an initialised one-rank process group, take every collective branch (SyncBN
# all-gather / all-reduce, bucketed gradient all-reduce, loss all-reduce) as if world > 1, so the
# multi-rank code runs (and is captured into HIP graphs) on a single GPU (tests/test_graph_gpu.py).
FORCE_COLLECTIVES = False


def collectives_on(world=None):
    """True when the data-parallel collective branches run: world > 1, or FORCE_COLLECTIVES with an
    initialised process group."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    w = dist.get_world_size() if world is None else world
    return w > 1 or FORCE_COLLECTIVES


def _world(sync):
    if sync and dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


# Per-rank row counts of a SyncBN batch, keyed by (local rows, world): data-parallel ranks see the
# same batch shape every step, so the counts are exchanged (and read on the host) once per shape.
_GLOBAL_ROWS = {}
_GLOBAL_TOTAL = {}


def bn_batch_stats(x, bn, sync):
    """Train-mode BatchNorm / SyncBatchNorm statistics of NHWC rows x: (mean, rstd, count), with the
    running statistics updated like torch (momentum, unbiased variance). With SyncBN over a
    multi-rank group the per-rank shifted sums are all-gathered into one [world, 3, C] buffer and
    merged on the device (K.bn_merge; torch SyncBatchNorm all-gathers (mean, invstd, count) the
    same way, torch/nn/modules/_functions.py)."""
    st = K.bn_stats(x)
    rows = x.shape[0]
    world = _world(sync)
    count = rows
    if sync and collectives_on(world):
        # gathered along dim 0 as [world * 3, C] (gloo splits the output along its first dim and
        # requires each piece to have the input's shape; RCCL takes either form)
        gathered = torch.empty((world * st.shape[0],) + tuple(st.shape[1:]), device=st.device, dtype=st.dtype)
        dist.all_gather_into_tensor(gathered, st)
        gathered = gathered.view((world,) + tuple(st.shape))
        counts = _GLOBAL_ROWS.get((rows, world))
        if counts is None:  # first batch of this shape: exchange the per-rank row counts once
            cnt = torch.tensor([float(rows)], device=x.device)
            counts = torch.empty(world, device=x.device)
            dist.all_gather_into_tensor(counts, cnt)
            _GLOBAL_ROWS[(rows, world)] = counts
        st = K.bn_merge(gathered, counts)
        total = _GLOBAL_TOTAL.get((rows, world))
        if total is None:  # one host read per batch shape, not one per BN layer per step
            total = _GLOBAL_TOTAL[(rows, world)] = int(counts.sum().item())
        count = total
    mean, rstd = K.bn_finalize(st, count, bn.eps, bn.momentum if bn.momentum is not None else 0.1, bn.running_mean,
                               bn.running_var)
    bn.num_batches_tracked.add_(1)
    return mean, rstd, count


# test-only probe (tests/test_dp_gpu.py): when a dict, bn_grad_stats records per BN layer (by id) the
# float64 sums [sum dy*xhat, sum dy, sum |dy*xhat|, sum |dy|] of the rows it reduces, from the same
# dy / x / mean / rstd its kernel reads
BN_PROBE = None


def bn_grad_stats(x, dy, mean, rstd, bn, sync):
    """BatchNorm backward statistics st2 = (sum dy, sum dy * xhat) of NHWC rows. Returns (st2 for the
    input gradient, dgamma, dbeta). The local statistics ARE this rank's beta / gamma gradients
    (SyncBatchNorm's backward forms grad_weight / grad_bias before its all-reduce,
    torch/nn/modules/_functions.py; DDP then averages them like every gradient) and are written
    straight into the flat gradient slots, laid out [beta | gamma] by train.fused_chains; under
    SyncBN an all-reduced copy feeds the input gradient."""
    out = gslot_rows(bn.bias, bn.weight) if bn is not None and bn.affine else None
    if BN_PROBE is not None and bn is not None:
        dyd = dy.double()
        t = dyd * ((x.double() - mean.double()) * rstd.double())
        BN_PROBE[id(bn)] = torch.stack([t.sum(0), dyd.sum(0), t.abs().sum(0), dyd.abs().sum(0)])
    st = K.bn_bwd_stats(x, dy, mean, rstd, out=out.view(2, -1) if out is not None else None)
    stg = st
    if sync and collectives_on():
        stg = st.clone()
        dist.all_reduce(stg)
    return stg, st[1], st[0]


def bn_forward(rows, bn, sync):
    """(mean, rstd, count) of a BatchNorm over NHWC rows: batch statistics in train mode (running statistics
    updated), the running statistics as a fixed affine in eval mode. bn_backward takes this triple back,
    with bn.training as it was at forward time."""
    if bn.training:
        return bn_batch_stats(rows, bn, sync)
    return bn.running_mean, torch.rsqrt(bn.running_var + bn.eps), rows.shape[0]


def bn_backward(dy, x, stats, gamma, bn, sync, training, relu_y=None, need_dx=True):
    """Backward of y = BN(x), or of y = relu(BN(x)) when its output relu_y is given (ReLU' applied to dy
    first): (dx, dgamma, dbeta). stats = (mean, rstd, count) and training are the forward's. Train mode
    takes the batch-statistics input gradient; in eval mode BN was a fixed per-channel affine and dx is
    dy * rstd * gamma. need_dx=False returns dx = None without launching it."""
    mean, rstd, count = stats
    if relu_y is not None:
        dy = K.relu_bwd(dy.contiguous(), relu_y)
    st2, dgamma, dbeta = bn_grad_stats(x, dy, mean, rstd, bn, sync)
    if not need_dx:
        dx = None
    elif training:
        dx = K.bn_bwd_apply(x, dy, mean, rstd, gamma, st2, count)
    else:
        dx = K.scale_mul(dy, colscale=rstd * gamma)
    return dx, dgamma, dbeta
