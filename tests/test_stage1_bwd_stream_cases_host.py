"""The cases of tests/golden/stage1_bwd_stream_cases.py proved on the host (numpy, and the library's size queries: no GPU).

  * every exact case meets the 2^24 abs-sum condition (asserted inside the generator), an fp32 evaluation in reversed
    order reproduces float64 exactly, and the float64 model of the kernel's tiles equals the reference;
  * on the real cases the same fp32 evaluation stays inside the gamma bound of ``bwd_bounds(splits=1)``;
  * each fault of the model (MUTANTS) changes the result of at least one exact case;
  * the workspace cap ``<= 64 B (a + b) + 2^20`` holds at every case and at the 1 M-entity shard shape, the size query
    follows the header's formula and returns 0 without a batch;
  * ``ops.stage1_backward_route`` takes the GEMM form at (2048, 200, 200, 200) and the stream form at (8192, 256, 512, 512).
"""
import numpy as np
import pytest

import exact_cases as ec
import stage1_bwd_stream_cases as sc

EXACT = [c for c in sc.CASES if c.exact]
REAL = [c for c in sc.CASES if not c.exact]
C5 = (8192, 256, 512, 512)


@pytest.fixture(scope="module")
def lib():
    from r_tucker_amd import _lib
    return _lib.load()


def test_the_list_covers_the_edges():
    names = [c.name for c in sc.CASES]
    assert len(names) == len(set(names))
    by = lambda br: [c for c in sc.CASES if c.branch.startswith(br)]      # noqa: E731
    assert [c.b for c in by("b edges")] == [1, 31, 33, 127, 128, 129, 257]
    assert [c.B for c in by("B edges")] == [1, 31, 33, 127, 128, 129, 257]
    assert [c.c for c in by("K edges")] == [1, 2, 7, 15, 16, 17, 33, 140]
    assert [c.a for c in by("a edges")] == [1, 2, 31, 33, 129]
    assert {c.regime for c in sc.CASES} == {"small", "wide12", "wide20", "real", "real_pow2"}
    assert any(c.b > 3 * sc.TILE_B for c in REAL) and any(c.B > 2 * sc.TILE_Q and c.b > 2 * sc.TILE_B for c in EXACT)


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_exact_case_fp32_reversed_and_model_equal_float64(case):
    ops = ec.bwd_operands(case)                           # asserts the 2^24 condition on g_core, g_R and g_S
    ref = ec.bwd_ref(*ops)
    got = ec.bwd_ref(*ops, dtype=np.float32, order="reversed", chunks=3)
    for g, e in zip(got, ref):
        assert g.dtype == np.float32 and np.array_equal(g.astype(np.float64), e)
    for g, e in zip(sc.model(*ops), ref):
        assert np.array_equal(g, e)


@pytest.mark.parametrize("case", REAL, ids=lambda c: c.name)
def test_real_case_fp32_reversed_inside_the_gamma_bound(case):
    ops = ec.bwd_operands(case)
    ref = ec.bwd_ref(*ops)
    bounds = ec.bwd_bounds(case, *ops, 1)
    got = ec.bwd_ref(*ops, dtype=np.float32, order="reversed", chunks=3)
    worst = max(float(np.max(np.abs(g.astype(np.float64) - e) / np.maximum(bd, np.finfo(np.float64).tiny)))
                for g, e, bd in zip(got, ref, bounds))
    print(f"\n[stage-1 bwd stream, host] {case.name}: fp32 reversed error / gamma bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_every_mutant_changes_an_exact_case(mutant):
    hit = []
    for case in EXACT:
        ops = ec.bwd_operands(case)
        ref = ec.bwd_ref(*ops)
        if any(not np.array_equal(g, e) for g, e in zip(sc.model(*ops, mutant=mutant), ref)):
            hit.append(case.name)
    print(f"\n[stage-1 bwd stream, host] mutant {mutant}: seen by {len(hit)} of {len(EXACT)} exact cases")
    assert hit, mutant


def test_workspace_cap_and_formula(lib):
    q = lib.rtk_query_bwd_stream_workspace_bytes
    for B, a, b, c in [(x.B, x.a, x.b, x.c) for x in sc.CASES] + [C5]:
        need = q(B, a, b, c)
        assert need == sc.workspace_model(B, a, b), (B, a, b, c)
        assert 0 < need <= 64 * B * (a + b) + (1 << 20), (B, a, b, c, need)
        assert need >= 4 * B * (2 * a + 2 * b)           # the gathered rows and the per-query rows are in it
    assert q(*C5) <= 404 << 20 and q(*C5) < lib.rtk_query_bwd_workspace_bytes(*C5) // 64
    assert lib.rtk_query_bwd_workspace_bytes(*C5) >= 2 * 8192 * 256 * 512 * 4


def test_size_query_is_zero_without_a_batch(lib):
    q = lib.rtk_query_bwd_stream_workspace_bytes
    assert q(0, 4, 4, 4) == 0 and q(-3, 4, 4, 4) == 0
    assert q(8, 0, 4, 4) == 0 and q(8, 4, 0, 4) == 0 and q(8, 4, 4, 0) == 0


def test_route_rule(lib, monkeypatch):
    from r_tucker_amd import ops
    assert ops._STAGE1_BWD_GEMM_BYTES == 1 << 30
    assert lib.rtk_query_bwd_workspace_bytes(2048, 200, 200, 200) <= 1 << 30
    assert ops.stage1_backward_route(2048, 200, 200, 200) == "gemm"
    assert ops.stage1_backward_route(*C5) == "stream"
    need = lib.rtk_query_bwd_workspace_bytes(70, 5, 64, 64)
    monkeypatch.setattr(ops, "_STAGE1_BWD_GEMM_BYTES", need)               # "stream" iff strictly above the limit
    assert ops.stage1_backward_route(70, 5, 64, 64) == "gemm"
    monkeypatch.setattr(ops, "_STAGE1_BWD_GEMM_BYTES", need - 1)
    assert ops.stage1_backward_route(70, 5, 64, 64) == "stream"
    monkeypatch.setattr(ops, "_STAGE1_BWD_GEMM_BYTES", 0)
    assert ops.stage1_backward_route(0, 5, 64, 64) == "gemm"               # an empty batch needs nothing
