"""tests/golden/ce_part_cases.py without a GPU: the blocks' float64 references add up to the whole-matrix reference of
ce_kernel_cases.stream_forward, the case list has the blocks the device test relies on, and every named mutant leaves
its bound by a factor of ten or more."""
import numpy as np
import pytest

import ce_kernel_cases as cc
import ce_part_cases as pc

by_name = dict(ids=lambda c: c.name)
SMALL = [c for c in pc.PART_CASES if c.case.N <= 95]


def test_the_case_list_has_the_blocks_the_device_test_needs():
    for c in pc.PART_CASES + [pc.MUTANT_CASE]:
        assert c.cuts[0] == 0 and c.cuts[-1] == c.case.N and list(c.cuts) == sorted(set(c.cuts))
    for c in pc.PART_CASES:
        assert all(x % 32 != 0 for x in c.cuts[1:-1]), c.name
    blocks = [(c.case, a, n) for c in pc.PART_CASES for a, n in c.blocks]
    assert any(n == 1 for _, _, n in blocks)                                    # a block of one row
    assert any(n == 31 and s.B == 1 and cc.splits_of(1) > 1 for s, _, n in blocks)  # more splits than tiles
    assert {(s.family, s.B, s.N, s.c) for s, _, _ in blocks} >= {("E", 33, 95, 20), ("G", 33, 95, 20), ("E", 70, 4099, 100),
                                                                 ("G", 70, 4099, 100), ("E", 70, 3003, 208),
                                                                 ("G", 70, 3003, 208), ("G", 31, 33, 4)}
    # query 0's dominant logit is in the last block and in no other
    for c in SMALL:
        data = cc.stream_operands(c.case)
        if c.case.N > 1:
            assert int(data.z[0].argmax()) == c.case.N - 1 and len(c.blocks) >= 2


@pytest.mark.parametrize("c", SMALL + [pc.MUTANT_CASE], **by_name)
def test_blocks_add_up_to_the_whole_matrix_reference(c):
    case = c.case
    data = cc.stream_operands(case)
    lse, rows = cc.stream_forward(case, data)[:2]
    refs = [pc.block_forward(case, data, a, n) for a, n in c.blocks]
    merged = pc.merge_lse([r["m"] for r in refs], [np.exp(r["lse"] - r["m"]) for r in refs])
    assert np.abs(merged - lse).max() <= 1e-13 * (1.0 + np.abs(lse).max())
    _, dt, eps = cc.consts64(case.N, case.eps)
    w = cc.weights(data.csr.stored(), dt, eps)
    total = w * merged + sum(r["lin"] for r in refs)
    assert np.abs(total - rows).max() <= 1e-12 * (1.0 + np.abs(rows).max())
    # a list with entries in two blocks, where the case has lists at all
    if len(c.blocks) >= 2 and data.csr.longest() >= 2:
        owners = [{int(np.searchsorted(c.cuts, t, side="right")) for t in data.csr.positives(d, case.N)} for d in range(case.B)]
        assert any(len(o) > 1 for o in owners)
    # the references pass their own verdict, and every bound is positive where something is summed
    for r in refs:
        ok, r_lse, r_lin = pc.block_forward_verdict(case, r, r["m"].astype(np.float32) if case.family == "E" else r["m"],
                                                    np.exp(r["lse"] - r["m"]), r["lin"])
        assert ok and r_lse <= 1e-3 and r_lin <= 1e-3
        assert (r["lse_b"] > 0).all()


def test_every_mutant_fails_by_a_factor_of_ten():
    c = pc.MUTANT_CASE
    case = c.case
    assert case.N == 64 and c.blocks == [(0, 32), (32, 32)] and case.eps == 0.5
    data = cc.stream_operands(case)
    assert 90.0 <= np.abs(data.z).max() <= 200.0
    refs = [pc.block_forward(case, data, a, n) for a, n in c.blocks]
    for mutant in ("t0_from_n_local", "n_d_from_the_block"):
        worst = 0.0
        for (a, n), r in zip(c.blocks, refs):
            bad = pc.block_forward(case, data, a, n, mutant=mutant)
            worst = max(worst, cc._ratio(np.abs(bad["lin"] - r["lin"]), r["lin_b"]))
        print(f"{mutant}: error / bound = {worst:.3g}")
        assert worst >= 10.0, mutant
    ms, ss = [r["m"] for r in refs], [np.exp(r["lse"] - r["m"]) for r in refs]
    lse, bound = pc.merged_lse_reference(c, data)
    assert cc._ratio(np.abs(pc.merge_lse(ms, ss) - lse), bound) <= 1e-3
    worst = cc._ratio(np.abs(pc.merge_lse(ms, ss, mutant="merge_without_maxima") - lse), bound)
    print(f"merge_without_maxima: error / bound = {worst:.3g}")
    assert worst >= 10.0
    assert set(pc.MUTANTS) == {"t0_from_n_local", "n_d_from_the_block", "merge_without_maxima"}
