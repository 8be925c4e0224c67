"""The table of tests/golden/*.npz: which generator call writes each fixture, and which fixtures it reads.

Plain data: importing it needs neither torch nor the reference (tests/test_golden_registry_cpu.py checks it
against the committed files). oracle/make_goldens.py runs the entries: each one alone, after torch.manual_seed(0),
with the fixtures it `needs` generated first into the same directory when they are absent. No fixture consumes
state left by another one: an entry lists several files only where one run produces them.
"""
from collections import namedtuple

Entry = namedtuple("Entry", "files call args kwargs needs")  # call: "<module>.<function>" under oracle/
ENTRIES = []


def _add(files, call, *args, needs=(), **kwargs):
    ENTRIES.append(Entry((files,) if isinstance(files, str) else tuple(files), call, args, kwargs, tuple(needs)))


# ---- blocks: name, model, stage, B, H, W, last
BLOCKS = [
    ("block_tiny_s0", "tiny", 0, 2, 12, 16, False),
    ("block_tiny_s1", "tiny", 1, 2, 11, 13, False),
    ("block_tiny_s3_last", "tiny", 3, 2, 5, 7, True),
    ("block_base_s0", "base", 0, 1, 16, 20, False),
    # the stage-0 plane of a 480x640 image (19,200 pixels): the fused ConvFFN's "auto" mode runs here
    ("block_base_s0_120x160", "base", 0, 1, 120, 160, False),
    ("block_base_s1", "base", 1, 2, 15, 20, False),
    ("block_base_s2", "base", 2, 2, 9, 10, False),
    ("block_base_s3", "base", 3, 2, 8, 10, False),
    ("block_base_s3_last", "base", 3, 2, 8, 10, True),
    ("block_large_s1", "large", 1, 1, 9, 11, False),
    ("block_large_s2", "large", 2, 1, 8, 9, False),
    # DFormer-Large at 530x730 (BASELINE config 5): stage 2 is 34x46, stage 3 17x23
    ("block_large_s2_34x46", "large", 2, 1, 34, 46, False),
    ("block_large_s3_17x23", "large", 3, 1, 17, 23, False),
]
BF16_BLOCKS = ("block_tiny_s1", "block_base_s0", "block_base_s1", "block_base_s2", "block_base_s3",
               "block_base_s3_last", "block_large_s2", "block_base_s0_120x160")
for b in BLOCKS:
    _add(b[0], "golden_blocks.golden_block", *b)
    if b[0] in BF16_BLOCKS:
        _add("bf16env_" + b[0], "golden_blocks.golden_block_bf16_env", *b, needs=[b[0]])
_add("block_tiny_s3_last_ye", "golden_blocks.golden_block", "block_tiny_s3_last_ye", "tiny", 3, 2, 5, 7, True,
     with_ye=True)
# DropPath with injected keep masks, one per DropPath call in the order of Block.forward
_add("block_droppath_base_s1", "golden_blocks.golden_block", "block_droppath_base_s1", "base", 1, 2, 9, 11, False,
     drop_prob=0.25, masks=[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 1.0]])

# ---- decoders
_add("nmf_train", "golden_decoders.golden_nmf", "nmf_train", 2, 64, 8, 10, True)
_add("nmf_eval", "golden_decoders.golden_nmf", "nmf_eval", 1, 64, 7, 9, False)
_add("ham_tiny", "golden_decoders.golden_ham", "ham_tiny", [64, 128, 256], 1, 6, 8)
_add("mlpdec_small", "golden_decoders.golden_mlpdec", "mlpdec_small", [32, 64, 128, 256], 2, 16, 20, embed=64)
_add("fcnhead_c128", "golden_decoders.golden_fcnhead", "fcnhead_c128", 2, 128, 37, 5, 7)
_add("fcnhead_c288", "golden_decoders.golden_fcnhead", "fcnhead_c288", 1, 288, 40, 3, 2)  # every pixel on the border
_add("uperhead_c32", "golden_decoders.golden_uperhead", "uperhead_c32", 2, [16, 32, 64, 96], 32,
     [(9, 13), (5, 7), (3, 4), (2, 2)], 1e-5)
_add("uperhead_c64", "golden_decoders.golden_uperhead", "uperhead_c64", 2, [32, 64, 128, 256], 64,
     [(12, 20), (6, 10), (3, 5), (2, 3)], 5e-6)

# ---- end to end, and the reference's own low-precision error on the same step
E2E = {
    "e2e_tiny_small": (("DFormer-Tiny", 2, 64, 96), {}),
    "e2e_base_small": (("DFormer-Base", 2, 64, 80), {}),
    "e2e_large_mlp_small": (("DFormer-Large", 1, 53, 73), dict(decoder="MLPDecoder", ncls=37)),
}
ENVS = [("bf16env_", "bfloat16", list(E2E)), ("fp32env_", None, list(E2E)),  # fp32env: the noise floor of the fp32 gates
        ("f16env_", "float16", ["e2e_large_mlp_small"])]  # train.py --amp, config 5
for n, (a, kw) in E2E.items():
    _add(n, "golden_e2e.golden_e2e", n, *a, **kw, **(dict(margin=3e-6) if n == "e2e_tiny_small" else {}))
for prefix, dtype, names in ENVS:
    for n in names:
        _add(prefix + n, "golden_e2e.golden_e2e_env", prefix, dtype, n, *E2E[n][0], needs=[n], **E2E[n][1])
_add("e2e_tiny_full_fwd", "golden_e2e.golden_e2e", "e2e_tiny_full_fwd", "DFormer-Tiny", 2, 480, 640, backward=False)
# the aux fixtures take their shape, input seed and (40 classes) main-path values from e2e_tiny_small
_add("e2e_tiny_aux37", "golden_e2e.golden_e2e_aux", "e2e_tiny_aux37", 37, needs=["e2e_tiny_small"])
_add("e2e_tiny_aux", "golden_e2e.golden_e2e_aux", "e2e_tiny_aux", 40, needs=["e2e_tiny_small"])
_add("e2e_tiny_uper", "golden_e2e.golden_e2e_uper", "e2e_tiny_uper")
_add("trav_expand_small", "golden_e2e.golden_expand", "trav_expand_small", 3, 12, 10, 6)
_add("trav_expand_full", "golden_e2e.golden_expand", "trav_expand_full", 2, 360, 640, 480)
_add("e2e_trav_small", "golden_e2e.golden_e2e_trav", "e2e_trav_small")
_add("e2e_fss_small", "golden_e2e.golden_fss")

# ---- evaluation
_add("msf_tiny_ham", "golden_eval.golden_msf", "msf_tiny_ham", "DFormer-Tiny", 2, 50, 70)
_add("msf_tiny_mlp", "golden_eval.golden_msf", "msf_tiny_mlp", "DFormer-Tiny", 1, 45, 61, decoder="MLPDecoder", ncls=37,
     embed=64)
_add("eval_tiny_ham", "golden_eval.golden_eval", "eval_tiny_ham", "DFormer-Tiny", 2, 50, 70, "ham", 40, 512)  # low-res 7x9, x8 head
_add("eval_tiny_mlp", "golden_eval.golden_eval", "eval_tiny_mlp", "DFormer-Tiny", 2, 50, 70, "MLPDecoder", 37, 64)  # 13x18, x4
# 1x2, 2x2 and 3x4 window grids, the last row / column of windows clamped; one file per image of batch 0
_add(["slide_tiny_ham", "slide_tiny_ham_img1"], "golden_eval.golden_slide", "slide_tiny_ham", "DFormer-Tiny", 2, 70, 90,
     "ham", 40, 512, (64, 64), 2 / 3, (0.75, 1.0, 1.5))
# scales 0.5 and 1.0 are smaller than the crop (1.0: 64x64 -> 64x96 changes the aspect ratio); 1.75 gives a 2x2 grid
_add("slide_tiny_mlp", "golden_eval.golden_slide", "slide_tiny_mlp", "DFormer-Tiny", 1, 45, 61, "MLPDecoder", 37, 64,
     (64, 96), 0.5, (0.5, 1.0, 1.75))

# ---- groups
_add("groups_base", "golden_e2e.golden_groups")

BY_FILE = {f: e for e in ENTRIES for f in e.files}


def order(files):
    """The entries that write `files`, each after the entries writing what it needs."""
    out = []

    def visit(e, path=()):
        if e in path:
            raise ValueError("dependency cycle through " + e.files[0])
        for n in e.needs:
            visit(BY_FILE[n], path + (e,))
        if e not in out:
            out.append(e)

    for f in files:
        visit(BY_FILE[f])
    return out
