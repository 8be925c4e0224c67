"""The kernel-variant ledger: every kernel instantiation of the built library, by name.

The library holds several hundred kernel instantiations, and host dispatch code picks one from shape,
dtype, alignment and size thresholds. This module lists them (the host launch stubs in the library's
symbol table, demangled and normalised to their template-id) and reads the launch tracer with the same
normalisation, so a test can say which instantiation a call ran and a ledger can say which ones no
test pins (tests/test_kernel_variants_cpu.py, tests/test_kernel_variants_gpu.py,
tests/kernel_variants_unpinned.txt).
"""
import ctypes
import ctypes.util
import functools
import os
import struct

STUB = "__device_stub__"
HERE = os.path.dirname(os.path.abspath(__file__))
UNPINNED_PATH = os.path.join(HERE, "kernel_variants_unpinned.txt")


def _symtab_names(path):
    """Names of the symbols in an ELF64 little-endian file's .symtab (falls back to .dynsym)."""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, f"{path}: not an ELF64 LE file"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    tables = [s for s in sections if s[1] == 2] or [s for s in sections if s[1] == 11]  # SHT_SYMTAB / SHT_DYNSYM
    assert tables, f"{path}: no symbol table (stripped?)"
    names = []
    for _, _, _, _, off, size, link, _, _, entsize in tables:
        stroff = sections[link][4]
        for o in range(off, off + size, entsize or 24):
            st_name, = struct.unpack_from("<I", data, o)
            if st_name:
                end = data.index(b"\0", stroff + st_name)
                names.append(data[stroff + st_name:end].decode())
    return names


_cxx = None


def demangle(mangled):
    """abi::__cxa_demangle of the C++ runtime this process already has (no external tool)."""
    global _cxx
    if _cxx is None:
        lib = None
        for cand in ("libstdc++.so.6", ctypes.util.find_library("stdc++"), "libc++abi.so.1"):
            try:
                lib = ctypes.CDLL(cand) if cand else None
            except OSError:
                lib = None
            if lib is not None and hasattr(lib, "__cxa_demangle"):
                break
        assert lib is not None, "no C++ runtime with __cxa_demangle to load"
        lib.__cxa_demangle.restype = ctypes.c_void_p
        lib.__cxa_demangle.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        libc = ctypes.CDLL(None)
        libc.free.argtypes = [ctypes.c_void_p]
        _cxx = (lib, libc)
    lib, libc = _cxx
    st = ctypes.c_int(0)
    p = lib.__cxa_demangle(mangled.encode(), None, None, ctypes.byref(st))
    assert st.value == 0 and p, f"cannot demangle {mangled!r} (status {st.value})"
    out = ctypes.string_at(p).decode()
    libc.free(p)
    return out


def _close(s, i, op, cl):
    """Index just past the bracket that closes s[i] == op."""
    depth = 0
    for j in range(i, len(s)):
        if s[j] == op:
            depth += 1
        elif s[j] == cl:
            depth -= 1
            if depth == 0:
                return j + 1
    raise ValueError(f"unbalanced {op}{cl} in {s!r}")


def normalise(demangled):
    """A demangled kernel (or launch stub) name -> its template-id: no stub prefix, no anonymous
    namespace, no return type, no parameter list. `void (anonymous namespace)::__device_stub__k<float, 4>(int)`
    and the tracer's `void (anonymous namespace)::k<float, 4>(int)` both give `k<float, 4>`."""
    s = demangled.replace("(anonymous namespace)::", "").replace(STUB, "")
    # the function name: the identifier that ends at the first '<' or '(' of nesting depth 0 after the return type
    depth, start = 0, 0
    for i, ch in enumerate(s):
        if ch in "<(" and depth == 0:
            end = _close(s, i, "<", ">") if ch == "<" else i
            return s[start:end].strip()
        if ch == " " and depth == 0:
            start = i + 1  # what came before was the return type (or part of it)
    return s[start:].strip()


@functools.lru_cache(maxsize=None)
def library_variants(path=None):
    """(normalised names, raw stub count): every kernel instantiation in the library."""
    if path is None:
        from dformer_amd import _lib
        path = _lib.LIB_PATH
    raw = [n for n in _symtab_names(path) if STUB in n]
    return sorted(normalise(demangle(n)) for n in raw), len(raw)


def read_unpinned(path=UNPINNED_PATH):
    """[(name, reason)] of tests/kernel_variants_unpinned.txt: `name  # reason` per line."""
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            name, sep, reason = line.partition("  # ")
            assert sep and reason.strip(), f"{path}:{ln}: want `name  # reason`, got {line!r}"
            out.append((name.strip(), reason.strip()))
    return out


class Trace:
    """`with Trace() as t: call()` records the kernels the call launched: t.names is the set of their
    normalised names, t.launched the list in launch order. The tracer is switched off on exit."""

    def __enter__(self):
        from dformer_amd import _lib
        self._lib = _lib
        self.names, self.launched = set(), []
        _lib.check(_lib.lib.dfm_trace_set(1, None), "dfm_trace_set")
        return self

    def __exit__(self, *exc):
        lib = self._lib.lib
        try:
            cap = 4096
            funcs = (ctypes.c_void_p * cap)()
            n = lib.dfm_trace_take(funcs, cap)
            assert n <= cap, f"{n} launches in one traced call"
            self.launched = [normalise(lib.dfm_kernel_name(funcs[i]).decode()) for i in range(n)]
            self.names = set(self.launched)
        finally:
            lib.dfm_trace_set(0, None)
        return False
