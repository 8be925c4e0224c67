"""oracle/golden_registry.py against the committed fixtures: every tests/golden/*.npz has exactly one generator
entry, every declared dependency is a fixture of the table, and the dependencies form no cycle. The table is
plain data: nothing of the reference (or of the generators, which import it) is loaded."""
import glob
import os
import types

import golden_registry as registry

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_golden_registry():
    # plain data: generators are named as strings, no module is imported
    assert [k for k, v in vars(registry).items() if isinstance(v, types.ModuleType)] == []
    for e in registry.ENTRIES:
        module, function = e.call.split(".")
        assert os.path.exists(os.path.join(os.path.dirname(registry.__file__), module + ".py")), e.call
    # the file names are the committed fixtures, each written by one entry
    files = [f for e in registry.ENTRIES for f in e.files]
    assert len(files) == len(set(files)), "a fixture is written by two entries"
    committed = {os.path.basename(p)[:-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "*.npz"))}
    assert set(files) == committed, sorted(set(files) ^ committed)
    # every dependency is a fixture of the table, written by another entry
    for e in registry.ENTRIES:
        assert all(n in registry.BY_FILE for n in e.needs), (e.files, e.needs)
        assert not set(e.needs) & set(e.files), e.files
    # no cycle: a full order exists (order() raises ValueError otherwise) and respects every dependency
    ordered = registry.order(list(registry.BY_FILE))
    assert len(ordered) == len(registry.ENTRIES)
    done = set()
    for e in ordered:
        assert set(e.needs) <= done, (e.files, e.needs)
        done |= set(e.files)
