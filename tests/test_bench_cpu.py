"""bench.py's command line and --dump-outputs writer (CPU; the timed step itself needs the GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench
from dformer_amd.segmentor import EncoderDecoder
from dformer_amd.train import FusedAdamW


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    a = parse(monkeypatch, "--full", "--table-out", "t.json", "--dump-outputs", "d")
    assert a.full is True and a.table_out == "t.json" and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [("--table-out", "t.json"), ("--steps", "0")])
def test_rejected_arguments(monkeypatch, argv):
    with pytest.raises(SystemExit) as e:
        parse(monkeypatch, *argv)
    assert e.value.code == 2


def test_dump_outputs(tmp_path, monkeypatch):
    """loss / params / grads as float32; arrays above DUMP_SAMPLE elements are cut to the same sorted
    positions on every call; smaller ones are written whole, in model.parameters() order."""
    torch.manual_seed(0)
    model = EncoderDecoder(cfg=bench.make_cfg("DFormer-Tiny", "ham", 40))
    opt = FusedAdamW(model, world=1, compute_dtype=torch.bfloat16)
    for g in opt.groups:
        g.grad.copy_(torch.arange(g.grad.numel(), dtype=torch.float32) % 1000)
    trainable = [p for p in model.parameters() if p.requires_grad]
    full = torch.cat([p.detach().reshape(-1) for p in trainable]).numpy()
    in_group = [p for p in trainable if any(p in g.slots for g in opt.groups)]
    assert len(in_group) < len(trainable)  # layer scales / custom LayerNorms are in no optimizer group

    monkeypatch.setattr(bench, "DUMP_SAMPLE", full.size)
    bench.dump_outputs(str(tmp_path / "whole"), model, opt, torch.tensor(1.25))
    got = {n: np.load(tmp_path / "whole" / f"{n}.npy") for n in ("loss", "params", "grads")}
    assert sorted(os.listdir(tmp_path / "whole")) == ["grads.npy", "loss.npy", "params.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].tolist() == [1.25]
    assert np.array_equal(got["params"], full)
    assert got["grads"].size == sum(p.numel() for p in in_group) == sum(g.grad.numel() for g in opt.groups)
    g0, (off, k) = next((g, g.slots[in_group[0]]) for g in opt.groups if in_group[0] in g.slots)
    assert np.array_equal(got["grads"][:k], g0.grad[off:off + k].numpy())

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 4096)
    bench.dump_outputs(str(tmp_path / "a"), model, opt, torch.tensor(1.25))
    bench.dump_outputs(str(tmp_path / "b"), model, opt, torch.tensor(1.25))
    a, b = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "b" / "params.npy")
    assert a.shape == (4096,) and np.array_equal(a, b)
    assert np.load(tmp_path / "a" / "grads.npy").shape == (4096,)
    gen = torch.Generator().manual_seed(8964)
    idx = torch.randperm(full.size, generator=gen)[:4096].sort().values.numpy()
    assert np.array_equal(a, full[idx])
