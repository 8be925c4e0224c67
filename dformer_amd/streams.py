"""Every stream this package creates for the training step, and the one fork / join idiom on them.

Roles (one stream per device and role):
  "ffn"       the RGB ConvFFN of a Block and the depth stem / downsample (encoder.py)
  "attn_bwd"  the RGB half of the attention backward (functional.AttentionFn)
  "wgrad"     a Block backward's grouped weight gradients of >= kernels.WG_STREAM_MIN_FLOPS
All of them carry gradient-writing kernels, so join_streams waits for each.
"""
import contextlib

import torch

_STREAMS = {}  # (device, role) -> stream, in creation order


def side_stream(dev, role):
    s = _STREAMS.get((dev, role))
    if s is None:
        s = _STREAMS[(dev, role)] = torch.cuda.Stream(device=dev)
    return s


@contextlib.contextmanager
def fork(side, reads=()):
    """The body runs on `side`, after `side` waits for what the current stream has issued so far.
    `reads`: tensors allocated on the current stream that the body reads (no reuse before it ran)."""
    side.wait_stream(torch.cuda.current_stream(side.device))
    with torch.cuda.stream(side):
        yield
    for t in reads:
        t.record_stream(side)


def join(side, made=()):
    """The current stream waits for `side`. `made`: tensors (or None) allocated inside the fork that
    are read on the current stream from here on."""
    cur = torch.cuda.current_stream(side.device)
    cur.wait_stream(side)
    for t in made:
        if t is not None:
            t.record_stream(cur)


def join_streams(main=None):
    """The current stream waits for everything issued so far on `main` (the stream the step's
    backward was started from) and on every side stream of this package, so a collective enqueued
    next sees every gradient slot complete whichever stream autograd ran its last hook on."""
    streams = ([main] if main is not None else []) + list(_STREAMS.values())
    if not streams:  # nothing issued off the current stream
        return
    cur = torch.cuda.current_stream()
    for s in streams:
        if s.device == cur.device and s != cur:
            cur.wait_stream(s)
