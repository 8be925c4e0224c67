"""Generate tests/golden/*.npz by running the READ-ONLY reference on CPU in float64.

TEST INFRASTRUCTURE. Run in the build container only:
    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens.py [--out DIR] [--list] [NAME-PREFIX ...]
    PYTHONDONTWRITEBYTECODE=1 python oracle/make_goldens.py compare DIR_A DIR_B
golden_registry.py is the table of fixtures; the generators are golden_blocks / golden_decoders / golden_e2e /
golden_eval.py over golden_common.py, which imports /root/reference through oracle/ref_shims (mmcv/mmengine
restatements) on first use and loads deterministic weights from oracle/gen.py. Nothing from the reference is
copied: the .npz files hold only arrays and name lists (inputs are regenerated from the seeds in gen.py).

Without NAME-PREFIX every fixture is written, otherwise those whose file name starts with one. --out defaults to
tests/golden; write elsewhere and `compare` against tests/golden to check a fixture without overwriting it. A
fixture that reads others (golden_registry: needs) reads them from --out, and they are generated first when
absent. `compare` reports per file `identical` or how many arrays differ and the worst max|a-b| / max|b|; it
applies no tolerance and fails only on a missing file or on differing keys, dtypes or shapes.
"""
import argparse
import glob
import importlib
import os
import sys
import time

import numpy as np

import golden_registry as registry


def generate(out, chosen):
    """Write the fixtures `chosen` (file names without .npz) into `out`, what they need first."""
    import torch
    import golden_common
    golden_common.OUT = out
    os.makedirs(out, exist_ok=True)
    for e in registry.order(chosen):
        if not set(e.files) & set(chosen) and all(os.path.exists(os.path.join(out, f + ".npz")) for f in e.files):
            continue  # a needed fixture that is already there
        t0 = time.time()
        golden_common.ref()
        torch.manual_seed(0)
        module, function = e.call.split(".")
        getattr(importlib.import_module(module), function)(*e.args, **e.kwargs)
        print(f"  {' '.join(e.files)}: {time.time() - t0:.1f}s")


def compare(dir_a, dir_b):
    names = sorted({os.path.basename(p) for d in (dir_a, dir_b) for p in glob.glob(os.path.join(d, "*.npz"))})
    bad = 0
    for n in names:
        pa, pb = os.path.join(dir_a, n), os.path.join(dir_b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            bad += 1
            print(f"{n}: MISSING in {dir_b if os.path.exists(pa) else dir_a}")
            continue
        a, b = np.load(pa), np.load(pb)
        if set(a.files) != set(b.files):
            bad += 1
            print(f"{n}: KEYS differ: {sorted(set(a.files) ^ set(b.files))[:6]}")
            continue
        ndiff, worst, mismatch = 0, 0.0, []
        for k in a.files:
            x, y = a[k], b[k]
            if x.dtype != y.dtype or x.shape != y.shape:
                mismatch.append(f"{k} {x.dtype}{x.shape} / {y.dtype}{y.shape}")
            elif x.tobytes() != y.tobytes():
                ndiff += 1
                if x.dtype.kind in "fiu" and x.size:
                    x, y = x.astype(np.float64), y.astype(np.float64)
                    worst = max(worst, np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
                else:
                    worst = np.inf
        if mismatch:
            bad += 1
            print(f"{n}: DTYPE/SHAPE differ: {'; '.join(mismatch[:4])}")
        elif ndiff:
            print(f"{n}: {ndiff} of {len(a.files)} arrays differ, worst max|a-b|/max|b| {worst:.3e}")
        else:
            print(f"{n}: identical")
    return 1 if bad else 0


def main():
    if sys.argv[1:2] == ["compare"]:
        p = argparse.ArgumentParser(prog="make_goldens.py compare")
        p.add_argument("dir_a")
        p.add_argument("dir_b")
        a = p.parse_args(sys.argv[2:])
        return compare(a.dir_a, a.dir_b)
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                 "tests", "golden"))
    p.add_argument("--list", action="store_true", help="print the fixtures, their generator calls and needs")
    p.add_argument("prefixes", nargs="*", metavar="NAME-PREFIX")
    a = p.parse_args()
    if a.list:
        for e in registry.ENTRIES:
            print(f"{' '.join(e.files)}: {e.call}" + (f" (needs {' '.join(e.needs)})" if e.needs else ""))
        return 0
    generate(a.out, [f for f in registry.BY_FILE if not a.prefixes or any(f.startswith(p) for p in a.prefixes)])
    return 0


if __name__ == "__main__":
    sys.exit(main())
