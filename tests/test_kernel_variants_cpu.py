"""The kernel-variant ledger (no GPU): every kernel instantiation of the built library is either
pinned by a case of tests/test_kernel_variants_gpu.py (which asserts, with the launch tracer, that
its call runs exactly the kernels it names) or listed in tests/kernel_variants_unpinned.txt with the
reason. An instantiation added to the library without a case, a stale unpinned line, and a case
dropped from the table all fail here."""
import kernel_variants as kv
import test_kernel_variants_gpu as cases

# Kernel families every instantiation of which a case must pin (dwconv.hip except ffn_dgrad_dw3_kernel,
# layernorm.hip, attention.hip, and dfm_gemm's four kernels), by template name.
FULL_FAMILIES = (
    "dw3_rows_bwd_kernel", "dw3_stream_bwd_kernel", "dw3_stream_fwd_kernel", "dw3_stream_wgrad_kernel",
    "dw7_bwd_fused_kernel", "dw7_lds_wgrad_kernel", "dw_tile_fwd_kernel",
    "ln_fwd_kernel", "ln_bwd_kernel", "ln_fwd_vec_kernel", "ln_bwd_vec_kernel",
    "pool7_fwd_kernel", "pool7_bwd_kernel", "pool7_fwd_vec_kernel", "pool7_bwd_vec_kernel",
    "bilinear_fwd_kernel", "bilinear_bwd_kernel", "bilinear_fwd_vec_kernel", "bilinear_bwd_vec_kernel",
    "attn_fwd_mfma_kernel", "attn_bwd_mfma_kernel", "attn_fwd_combine_v4_kernel", "attn_dq_reduce_v4_kernel",
    "attn_fwd_chunk_kernel", "attn_fwd_combine_kernel", "attn_bwd_chunk_kernel", "attn_dq_reduce_kernel",
    "head_repack_kernel", "head_repack4_kernel",
    "gemm_kernel", "gemm_glds_kernel", "gemm_wide_kernel", "splitk_reduce_kernel")
# The stated exceptions. No call can reach these four: a 16-bit row of 4 vectors per lane has 1544..2048
# channels, and dfm_layernorm_fwd / dfm_layernorm_bwd reject C > 1024.
UNREACHABLE = frozenset(f"ln_{d}_vec_kernel<{t}, 64, 4>" for d in ("fwd", "bwd") for t in ("unsigned short", "f16_t"))
# The families hold 337 instantiations (704 in the library); with the four exceptions and the kernels
# pinned beyond the families, the unpinned file stays within the 361 lines the ledger was set up with.
FAMILY_COUNT = 337
UNPINNED_CAP = 361
# cases per family label of the table (attention.hip holds pool7, bilinear and the pooled attention)
CASE_COUNT = {"gemm": 239, "dwconv": 78, "attention": 52, "layernorm": 31, "elementwise": 8}


def template_name(name):
    return name.split("<", 1)[0]


def test_library_names_are_unique():
    names, raw = kv.library_variants()
    assert raw > 0
    assert len(names) == raw
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, f"two kernels share a name (a launch trace cannot tell them apart): {dup}"


def test_normalise():
    f = kv.normalise
    assert f("void (anonymous namespace)::__device_stub__k<float, 4>(int, float const*)") == "k<float, 4>"
    assert f("void (anonymous namespace)::k<unsigned short, 3, false>((anonymous namespace)::Args)") == \
        "k<unsigned short, 3, false>"
    assert f("void plain_kernel(int)") == "plain_kernel"
    assert f("__device_stub__partial_sum_kernel<2>(int, long)") == "partial_sum_kernel<2>"


def test_ledger_is_exact():
    library = set(kv.library_variants()[0])
    declared = set(cases.declared())
    unpinned = [n for n, _ in kv.read_unpinned()]
    assert len(unpinned) == len(set(unpinned)), "a name is listed twice in the unpinned file"
    both = declared & set(unpinned)
    assert not both, f"pinned by a case and still listed as unpinned: {sorted(both)}"
    missing = library - declared - set(unpinned)
    assert not missing, f"in the library, neither pinned nor listed as unpinned: {sorted(missing)}"
    gone = (declared | set(unpinned)) - library
    assert not gone, f"not in the library (renamed or removed?): {sorted(gone)}"


def test_case_table_is_whole():
    """Several cases may pin one kernel (aligned and misaligned operands, several N), so a case that goes
    missing need not unpin a name: the table's size per family is stated here."""
    ids = [c.id for c in cases.CASES]
    assert len(ids) == len(set(ids))
    assert all(c.names for c in cases.CASES)
    count = {}
    for c in cases.CASES:
        count[c.family] = count.get(c.family, 0) + 1
    assert count == CASE_COUNT, count


def test_families_are_pinned_in_full():
    library = kv.library_variants()[0]
    family = [n for n in library if template_name(n) in FULL_FAMILIES]
    assert len(family) == FAMILY_COUNT, len(family)
    assert UNREACHABLE <= set(family)
    unpinned = [n for n, _ in kv.read_unpinned()]
    stray = sorted(n for n in unpinned if template_name(n) in FULL_FAMILIES and n not in UNREACHABLE)
    assert not stray, f"must be pinned by a case, not listed as unpinned: {stray}"
    assert len(unpinned) <= UNPINNED_CAP, len(unpinned)
