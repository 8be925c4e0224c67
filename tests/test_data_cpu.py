"""The input-pipeline library without a GPU: libdformer_data.so exports what include/dformer_data.h declares and
what dformer_amd/data.py binds, holds exactly the kernels listed here, rejects bad arguments before any launch,
and TrainPre.draw makes the reference's random draws in the reference's order."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest
import torch

import kernel_variants as kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dformer_data.h")

# Every kernel instantiation of libdformer_data.so, with the case of tests/test_data_gpu.py that runs it.
KERNELS = [
    "train_pre_kernel<1>",  # test_scales (1-channel modal), test_identity, test_small_image_odd_pad, test_graph_replay
    "train_pre_kernel<3>",  # test_modal_three_channels, test_options[all_three_channel_modal]
]


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\*)\s+(dfd_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        decls[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return decls


def test_binding_signatures_match_header():
    from dformer_amd import data
    d = declared()
    assert d == {"dfd_last_error": 0, "dfd_abi_version": 0, "dfd_train_pre": 9}
    assert set(d) == set(data._SIGS), set(d) ^ set(data._SIGS)
    for name, n in d.items():
        assert len(data._SIGS[name][1]) == n, (name, n, len(data._SIGS[name][1]))
    raw = ctypes.CDLL(data.LIB_PATH)
    for name in d:
        assert hasattr(raw, name), name
    assert data.lib.dfd_abi_version() == 1 == data.ABI_VERSION
    src = open(HEADER).read()
    assert f"#define DFD_MAX_DIM {data.MAX_DIM}\n" in src and f"#define DFD_MAX_SCALED {data.MAX_SCALED}\n" in src


def test_library_kernels_and_symbols():
    from dformer_amd import data
    names, raw = kv.library_variants(data.LIB_PATH)
    assert raw == len(names) and names == sorted(KERNELS), names
    assert len(names) <= 4
    symbols = kv._symtab_names(data.LIB_PATH)
    assert not [s for s in symbols if s.startswith("dfm_")], "the data library defines no dfm_* symbol"
    assert not hasattr(ctypes.CDLL(data.LIB_PATH), "dfm_abi_version")


def test_desc_layout_matches_c_struct(tmp_path):
    import shutil
    from dformer_amd import data
    assert ctypes.sizeof(data.PreDesc) == 8 * 4 + 12 * 4
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    names = [f[0] for f in data.PreDesc._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(DfdPreDesc));' % HEADER
    for n in names:
        src += 'printf(" %%zu", offsetof(DfdPreDesc, %s));' % n
    src += "return 0;}\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "t")], capture_output=True, text=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(data.PreDesc)
    assert vals[1:] == [getattr(data.PreDesc, n).offset for n in names]


def test_loader_refuses_another_abi():
    from dformer_amd import data

    class Stub:
        @staticmethod
        def dfd_abi_version():
            return 2

    with pytest.raises(ImportError) as e:
        data.check_abi(Stub)
    msg = str(e.value)
    assert "2" in msg and str(data.ABI_VERSION) in msg and data.LIB_PATH in msg
    data.check_abi(data.lib)


def test_import_maps_one_library_each():
    """import dformer_amd.segmentor maps the model library alone; importing dformer_amd.data maps the second."""
    code = ("import dformer_amd.segmentor\n"
            "m = open('/proc/self/maps').read()\n"
            "print(int('libdformer_hip.so' in m), int('libdformer_data.so' in m))\n"
            "import dformer_amd.data\n"
            "print(int('libdformer_data.so' in open('/proc/self/maps').read()))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["1", "0", "1"], out


# ---------------------------------------------------------------- draw

class RecordingRng:
    """Replays scripted answers and records every call with its arguments."""

    def __init__(self, randoms, choices, randints):
        self.randoms, self.choices, self.randints = list(randoms), list(choices), list(randints)
        self.calls = []

    def random(self):
        self.calls.append(("random",))
        return self.randoms.pop(0)

    def choice(self, seq):
        self.calls.append(("choice", tuple(seq)))
        return self.choices.pop(0)

    def randint(self, a, b):
        self.calls.append(("randint", a, b))
        return self.randints.pop(0)


def test_draw_call_order():
    from dformer_amd.data import TrainPre
    scales = [0.5, 1.0, 1.75]
    pre = TrainPre([0.485, 0.456, 0.406], [0.229, 0.224, 0.225], (24, 40), scales)
    # sample 0: mirrored, scale 1.75 -> 54 x 78, both larger than the crop; sample 1: scale 0.5 -> 15 x 22, no
    # randint at all; sample 2: scale 1.0 -> 31 x 45, both larger; random() == 0.5 mirrors (>=)
    rng = RecordingRng([0.9, 0.1, 0.5], [1.75, 0.5, 1.0], [31, 39, 0, 6])
    p = pre.draw(3, (31, 45), rng)
    assert p.dtype == torch.int32 and tuple(p.shape) == (3, 8) and not p.is_cuda
    assert p.tolist() == [[1, 54, 78, 31, 39, 0, 0, 0], [0, 15, 22, 0, 0, 0, 0, 0], [1, 31, 45, 0, 6, 0, 0, 0]]
    s = tuple(scales)
    assert rng.calls == [("random",), ("choice", s), ("randint", 0, 54 - 24 + 1), ("randint", 0, 78 - 40 + 1),
                         ("random",), ("choice", s),
                         ("random",), ("choice", s), ("randint", 0, 31 - 24 + 1), ("randint", 0, 45 - 40 + 1)]
    # only the height is larger than the crop: one randint; no scales: no choice
    pre = TrainPre(0.5, 0.25, (24, 45), None)
    rng = RecordingRng([0.2], [], [8])
    assert pre.draw(1, (31, 45), rng).tolist() == [[0, 31, 45, 8, 0, 0, 0, 0]]
    assert rng.calls == [("random",), ("randint", 0, 8)]


def test_draw_matches_restatement():
    from dformer_amd.data import TrainPre
    scales, (H0, W0), (ch, cw) = [0.5, 0.75, 1, 1.25, 1.5, 1.75], (48, 64), (40, 56)
    got = TrainPre(0.5, 0.25, (ch, cw), scales).draw(64, (H0, W0), random.Random(1234))
    rng, want = random.Random(1234), []
    for _ in range(64):
        flip = 1 if rng.random() >= 0.5 else 0
        s = rng.choice(scales)
        sh, sw = int(H0 * s), int(W0 * s)
        pos_h = rng.randint(0, sh - ch + 1) if sh > ch else 0
        pos_w = rng.randint(0, sw - cw + 1) if sw > cw else 0
        want.append([flip, sh, sw, pos_h, pos_w, 0, 0, 0])
    assert got.tolist() == want
    assert {r[0] for r in want} == {0, 1} and len({r[1] for r in want}) == len(scales)
    from dformer_amd.data import check_params
    check_params(got, 64)  # what draw returns passes the host range check, the randint quirk included


# ---------------------------------------------------------------- validation before any launch

GOOD = dict(B=2, H0=31, W0=45, ch=24, cw=40, modal_channels=1, bgr=0, transform_gt=0)


def make_desc(**kw):
    from dformer_amd import data
    f3 = ctypes.c_float * 3
    vals = dict(GOOD, mean=f3(0.5, 0.5, 0.5), std=f3(0.25, 0.25, 0.25), modal_mean=f3(0.5, 0.5, 0.5),
                modal_std=f3(0.25, 0.25, 0.25))
    vals.update(kw)
    return data.PreDesc(**vals)


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-1), dict(H0=0), dict(W0=-5), dict(ch=0), dict(cw=-1),
                                 dict(H0=16385), dict(ch=16385), dict(cw=16385), dict(modal_channels=2),
                                 dict(modal_channels=0), dict(std=(ctypes.c_float * 3)(0.25, 0.0, 0.25)),
                                 dict(modal_std=(ctypes.c_float * 3)(-1.0, 1.0, 1.0)), "null_rgb", "null_params",
                                 "null_out_label", "null_desc"])
def test_bad_descriptor_is_rejected(bad):
    """Status -1 with a message, before anything is launched: the pointers are never dereferenced."""
    from dformer_amd import data
    fake = ctypes.c_void_p(1 << 20)
    args = [make_desc(**bad) if isinstance(bad, dict) else make_desc()] + [fake] * 7 + [None]
    if bad == "null_rgb":
        args[1] = None
    elif bad == "null_params":
        args[4] = None
    elif bad == "null_out_label":
        args[7] = None
    elif bad == "null_desc":
        args[0] = None
    st = data.lib.dfd_train_pre(*args)
    assert st == -1
    assert data.lib.dfd_last_error().startswith(b"dfd_train_pre: ")
    with pytest.raises(RuntimeError):
        data.check(st, "dfd_train_pre")


@pytest.mark.parametrize("row", [
    [2, 31, 45, 0, 0, 0, 0, 0],     # flip not 0 / 1
    [-1, 31, 45, 0, 0, 0, 0, 0],
    [0, 31, 45, 31, 0, 0, 0, 0],    # pos_h >= sh
    [0, 31, 45, 0, 45, 0, 0, 0],    # pos_w >= sw
    [0, -31, 45, 0, 0, 0, 0, 0],    # negative sizes
    [0, 31, -45, 0, 0, 0, 0, 0],
    [0, 31, 45, -1, 0, 0, 0, 0],    # negative position
    [0, 32769, 45, 0, 0, 0, 0, 0],  # above DFD_MAX_SCALED
    [0, 31, 45, 0, 0, 0, 1, 0],     # reserved column
])
def test_bad_cpu_params_are_rejected(row):
    """A CPU params tensor is range-checked on the host: ValueError before the device tensors are even looked at."""
    from dformer_amd.data import TrainPre, check_params
    params = torch.tensor([[0, 31, 45, 0, 0, 0, 0, 0], row], dtype=torch.int32)
    with pytest.raises(ValueError, match=r"params\[1\]"):
        check_params(params, 2)
    pre = TrainPre(0.5, 0.25, (24, 40), None)
    u8 = torch.zeros(2, 31, 45, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"params\[1\]"):
        pre(u8, u8[..., 0].contiguous(), u8[..., 0].contiguous(), params)


def test_cpu_params_shape_and_dtype():
    from dformer_amd.data import check_params
    ok = torch.tensor([[0, 31, 45, 30, 44, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32)
    check_params(ok, 2)  # the last row / column as position, and an empty scaled image (padding only), are legal
    with pytest.raises(ValueError):
        check_params(ok, 3)
    with pytest.raises(ValueError):
        check_params(ok.long(), 2)
    with pytest.raises(ValueError):
        check_params(ok[:, :5].contiguous(), 2)


def test_constructor_arguments():
    from dformer_amd.data import TrainPre, ValPre
    pre = TrainPre([0.485, 0.456, 0.406], [0.229, 0.224, 0.225], (480, 640), None)
    assert pre.modal_mean == pre.mean and pre.modal_std == pre.std  # the reference's sign=False
    pre = ValPre([0.485, 0.456, 0.406], [0.229, 0.224, 0.225], [0.48], 0.28)
    assert pre.modal_mean == [0.48] * 3 and pre.modal_std == [0.28] * 3
    with pytest.raises(ValueError):
        TrainPre([0.5, 0.5], 0.25, (24, 40), None)
    with pytest.raises(ValueError):
        TrainPre(0.5, [0.25, 0.0, 0.25], (24, 40), None)
