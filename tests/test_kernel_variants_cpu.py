"""The kernel-variant ledger (no GPU): every kernel instantiation of the built library is either
pinned by a case of tests/test_kernel_variants_gpu.py or tests/test_kernel_variants_tier2_gpu.py (which
assert, with the launch tracer, that a call runs exactly the kernels it names) or listed in
tests/kernel_variants_unpinned.txt with the reason. An instantiation added to the library without a
case, a stale unpinned line, and a case dropped from either table all fail here."""
import kernel_variants as kv
import test_kernel_variants_gpu as tier1
import test_kernel_variants_tier2_gpu as tier2

CASES = tier1.CASES + tier2.CASES


def declared():
    return tier1.declared() | tier2.declared()


# Kernel families every instantiation of which a case must pin, by template name: dwconv.hip except
# ffn_dgrad_dw3_kernel, layernorm.hip, attention.hip and dfm_gemm's four kernels (tier 1); convffn.hip's
# forward and dhpre kernels, conv.hip, elementwise.hip's reductions, elementwise / BatchNorm / cast / pack /
# NMF / softmax kernels, the non-finite scan and the grouped GEMM launches (tier 2).
FULL_FAMILIES = (
    "dw3_rows_bwd_kernel", "dw3_stream_bwd_kernel", "dw3_stream_fwd_kernel", "dw3_stream_wgrad_kernel",
    "dw7_bwd_fused_kernel", "dw7_lds_wgrad_kernel", "dw_tile_fwd_kernel",
    "ln_fwd_kernel", "ln_bwd_kernel", "ln_fwd_vec_kernel", "ln_bwd_vec_kernel",
    "pool7_fwd_kernel", "pool7_bwd_kernel", "pool7_fwd_vec_kernel", "pool7_bwd_vec_kernel",
    "bilinear_fwd_kernel", "bilinear_bwd_kernel", "bilinear_fwd_vec_kernel", "bilinear_bwd_vec_kernel",
    "attn_fwd_mfma_kernel", "attn_bwd_mfma_kernel", "attn_fwd_combine_v4_kernel", "attn_dq_reduce_v4_kernel",
    "attn_fwd_chunk_kernel", "attn_fwd_combine_kernel", "attn_bwd_chunk_kernel", "attn_dq_reduce_kernel",
    "head_repack_kernel", "head_repack4_kernel",
    "gemm_kernel", "gemm_glds_kernel", "gemm_wide_kernel", "splitk_reduce_kernel",
    "ffn_fwd_kernel", "ffn_dhpre_kernel",
    "im2col_vec_kernel", "im2col_gen_kernel", "im2col_s1_kernel", "col2im_vec_kernel", "col2im_s1_kernel",
    "col2im_gen_kernel", "weight_pack_kernel", "weight_unpack_kernel",
    "ew2d_kernel", "ew2d_vec_kernel", "colred_kernel", "colred_vec_kernel", "bn_apply_kernel", "bn_apply_vec_kernel",
    "bn_bwd_apply_kernel", "bn_bwd_apply_vec_kernel", "bn_finalize_kernel", "bn_merge_kernel", "cast_kernel",
    "pack_slices_kernel", "pack_slices_vec_kernel", "nonfinite_kernel", "partial_sum_group_kernel",
    "softmax_rows_kernel", "softmax_rows_bwd_kernel", "nmf_update_kernel", "nmf_update_bwd_kernel",
    "nmf_update_mm_kernel", "nmf_update_bwd_mm_kernel",
    "gemm_group_kernel", "gemm_glds_group_kernel", "splitk_reduce_group_kernel")
# The stated exceptions, each verified in the host code.
_T3 = ("float", "unsigned short", "f16_t")
_T2 = _T3[1:]
_IM2COL = ("float, float", "float, unsigned short", "unsigned short, unsigned short", "unsigned short, float",
           "float, f16_t", "f16_t, f16_t")
UNREACHABLE = frozenset(
    # a 16-bit row of 4 vectors per lane has 1544..2048 channels; dfm_layernorm_fwd / _bwd reject C > 1024
    [f"ln_{d}_vec_kernel<{t}, 64, 4>" for d in ("fwd", "bwd") for t in _T2] +
    # ffn_fwd_launch: C = 32 takes the 8 x 8 tile with the GELU outputs and the 8 x 16 tile without them;
    # ffn_fwd_launch_t instantiates both booleans for both tiles
    [f"ffn_fwd_kernel<{t}, 32, 32, 8, 16, true>" for t in _T2] +
    [f"ffn_fwd_kernel<{t}, 32, 32, 8, 8, false>" for t in _T2] +
    # mode 1 is dfm_bn_stats alone (no second operand); mode 2 is dfm_bn_bwd_stats alone (null dy rejected)
    [f"colred_vec_kernel<{t}, 1, true>" for t in _T3] + [f"colred_vec_kernel<{t}, 2, false>" for t in _T3] +
    # conv.hip's 64-bit index twins: taken from 2^31 work items of 8 elements each (tens of GiB of operands)
    [f"im2col_{k}_kernel<{p}, long>" for k in ("vec", "gen") for p in _IM2COL] +
    [f"{k}_kernel<{t}, long>" for k in ("col2im_vec", "im2col_s1", "col2im_s1") for t in _T3])
# The families hold 513 of the library's 695 instantiations; the unpinned file holds the 35 exceptions and the
# 171 kernels of the families left to their own tests.
FAMILY_COUNT = 513
UNPINNED_CAP = 206
# cases per family label of the two tables (attention.hip holds pool7, bilinear and the pooled attention)
CASE_COUNT = {"gemm": 257, "dwconv": 78, "attention": 52, "layernorm": 31, "elementwise": 164, "conv": 176,
              "convffn": 36}


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
    pinned = set(declared())
    unpinned = [n for n, _ in kv.read_unpinned()]
    assert len(unpinned) == len(set(unpinned)), "a name is listed twice in the unpinned file"
    both = pinned & set(unpinned)
    assert not both, f"pinned by a case and still listed as unpinned: {sorted(both)}"
    missing = library - pinned - set(unpinned)
    assert not missing, f"in the library, neither pinned nor listed as unpinned: {sorted(missing)}"
    gone = (pinned | set(unpinned)) - library
    assert not gone, f"not in the library (renamed or removed?): {sorted(gone)}"


def test_case_table_is_whole():
    """Several cases may pin one kernel (aligned and misaligned operands, several N), so a case that goes
    missing need not unpin a name: the table's size per family is stated here."""
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    assert all(c.names for c in CASES)
    count = {}
    for c in CASES:
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
