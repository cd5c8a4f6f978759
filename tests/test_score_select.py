"""The fp32 score-kernel choice as the library exports it (rtk_score_kernel_f32, rtk_score_fifth_group_columns_f32):
host-only, no device touched.  Pinned to facts, not to a restatement of the rule: bench.py's kernel label (which
bench.py keeps in its own copy) and the fifth-group column counts of known shapes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from r_tucker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):   # build in-tree (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["bash", os.path.join(ROOT, "r-tucker_amd", "csrc", "build.sh")], check=True)
    return _lib.load()


NAMES = {0x100: "score_cg_kernel", 0x200: "score_ws_kernel", 0x300: "score_split_kernel"}


@pytest.mark.parametrize("c", [4, 200, 208, 209, 210, 512])
def test_kernel_choice_matches_the_bench_label(lib, monkeypatch, c):
    import bench
    monkeypatch.delenv("RTK_SCORE_KERNEL", raising=False)
    for N in (14951, 18400, 18432, 20000, 40943, 40960, 40961, 46000, 100000):
        assert NAMES[lib.rtk_score_kernel_f32(N, c, 0)] == bench.score_kernel_name(N, c), (N, c)


def test_known_choices(lib):
    from r_tucker_amd import _lib as L
    assert lib.rtk_score_kernel_f32(40943, 200, 0) == L.RTK_SCORE_KERNEL_CG       # WN18RR
    assert lib.rtk_score_kernel_f32(18400, 200, 0) == L.RTK_SCORE_KERNEL_WS       # 575 groups
    assert lib.rtk_score_kernel_f32(18432, 200, 0) == L.RTK_SCORE_KERNEL_CG       # 576 groups
    assert lib.rtk_score_kernel_f32(40961, 200, 0) == L.RTK_SCORE_KERNEL_WS       # 1281 groups: two sets per workgroup
    assert lib.rtk_score_kernel_f32(40943, 210, 0) == L.RTK_SCORE_KERNEL_V3       # c % 4 != 0
    assert lib.rtk_score_kernel_f32(40943, 212, 0) == L.RTK_SCORE_KERNEL_V3       # c > 208


def test_hints_override_the_shape_rule(lib):
    from r_tucker_amd import _lib as L
    for N in (100, 20000, 40943, 100000):
        for hint in (L.RTK_SCORE_KERNEL_CG, L.RTK_SCORE_KERNEL_WS, L.RTK_SCORE_KERNEL_V3):
            assert lib.rtk_score_kernel_f32(N, 200, hint) == hint, (N, hint)
        # a hinted kernel that does not cover the shape: v3 has the c % 4 != 0 and c > 208 paths
        for hint in (L.RTK_SCORE_KERNEL_CG, L.RTK_SCORE_KERNEL_WS):
            assert lib.rtk_score_kernel_f32(N, 210, hint) == L.RTK_SCORE_KERNEL_V3
            assert lib.rtk_score_kernel_f32(N, 256, hint) == L.RTK_SCORE_KERNEL_V3
    # the sigmoid bits do not change the choice
    assert lib.rtk_score_kernel_f32(40943, 200, L.RTK_SCORE_SIGMOID | L.RTK_SCORE_SIGMOID_FAST) == L.RTK_SCORE_KERNEL_CG


def test_fifth_group_columns(lib):
    from r_tucker_amd import _lib as L
    from r_tucker_amd.ops import cg_fifth_group_columns
    assert lib.rtk_score_fifth_group_columns_f32(20000, 200, 0, None) == 0     # <= 1024 groups: no set of five
    # WN18RR: 1280 groups, 256 sets of five; the last fifth group holds the 15 columns of the ragged last group
    assert lib.rtk_score_fifth_group_columns_f32(40943, 200, 0, None) == 8175
    m = cg_fifth_group_columns(40943, 200)
    assert m.dtype == bool and m.shape == (40943,) and int(m.sum()) == 8175
    assert m[128:160].all() and not m[:128].any() and m[-15:].all() and not m[-47:-15].any()
    # 3125 groups: the ws kernel without a hint, 768 sets of four and five under the cg hint
    assert lib.rtk_score_fifth_group_columns_f32(100000, 200, 0, None) == 0
    assert not cg_fifth_group_columns(100000, 200).any()
    n = lib.rtk_score_fifth_group_columns_f32(100000, 200, L.RTK_SCORE_KERNEL_CG, None)
    assert n > 0 and int(cg_fifth_group_columns(100000, 200, L.RTK_SCORE_KERNEL_CG).sum()) == n
    assert lib.rtk_score_fifth_group_columns_f32(40943, 200, L.RTK_SCORE_KERNEL_WS, None) == 0
    mask = np.full(64, 7, dtype=np.uint8)
    assert lib.rtk_score_fifth_group_columns_f32(64, 200, 0, mask.ctypes.data) == 0 and not mask.any()


def test_bad_shapes_are_argument_errors(lib):
    for N, c in ((0, 200), (-5, 200), (1000, 0), (1000, 513), (1 << 31, 200)):
        assert lib.rtk_score_kernel_f32(N, c, 0) == -1
        assert lib.rtk_score_fifth_group_columns_f32(N, c, 0, None) == -1
    assert b"outside the split-fp16 kernels' shapes" in lib.rtk_last_error_string()
