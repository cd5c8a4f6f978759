"""The method of tests/test_gpu_bce_stream_bf16_kernels.py, proved without a GPU on the cases of
tests/golden/bce_stream_bf16_cases.py:

  * the fp32 numpy emulation of each operand route of the two tile products (x as fp16 hi/lo against one fp16 plane of
    O; x as three bf16 terms against O as it is) stays within the derived bounds of rows, dv and gO on every case, also
    with every exponential moved one ulp up or down;
  * every named mutant is outside its bound on at least one case, judged by the verdict function the GPU test uses; the
    two block mutants leave the doubled bound of the block form by a factor of ten or more on the n_ent = 64 case;
  * the conditions the derivation states hold: O exact in bf16, v with full mantissas where the family is not exact,
    exact logits in families E and S, no logit where saturation is ambiguous, |z| + dz <= 15 outside S.
"""
import functools

import numpy as np
import pytest

import bce_stream_bf16_cases as bb
import bce_stream_cases as bs
import ce_kernel_cases as cc

by_name = dict(ids=lambda c: c.name)
ALL_CASES = bb.CASES + [bb.MUTANT_PART.case] + sorted({p.case for p in bb.PART_CASES} - set(bb.CASES), key=lambda c: c.name)


@functools.lru_cache(maxsize=None)
def setup(case):
    data = bb.operands(case)
    bb.assert_unambiguous(case, data)               # before anything is judged (and before anything goes to a GPU)
    return data, {mode: bb.bounds(case, data, mode == "fast") for mode in bb.MODES}


# ------------------------------------------------------------------------------------- emulations pass ----
@pytest.mark.parametrize("route", bb.ROUTES)
@pytest.mark.parametrize("case", ALL_CASES, **by_name)
def test_emulation_within_bounds(case, route):
    data, refs = setup(case)
    for mode in bb.MODES:
        for perturb in (0, 1, -1):
            r = bb.verdict(refs[mode], *bb.emul(case, data, mode == "fast", route, perturb))
            print(f"\n[bce stream bf16, emulated] {case.name} {route} {mode} {perturb:+d}: error / bound = {r[0]:.4f} (rows), "
                  f"{r[1]:.4f} (dv), {r[2]:.4f} (gO)")
            assert max(r) <= 1.0


def test_the_float64_reference_passes_its_own_verdict():
    for case in (bb.S_CASES[0], bb.SIGMA6_CASE):
        data, refs = setup(case)
        ref = refs["fast"]
        assert max(bb.verdict(ref, ref["rows"], ref["dv"].astype(np.float32), ref["gO"].astype(np.float32))) <= 1.0
        assert bb.reference(case, data, cuts=(0, 40, case.N))["rows"] == pytest.approx(ref["rows"], rel=1e-13)


def test_the_reference_takes_the_rounded_v_for_the_logits_and_the_unrounded_v_for_gO():
    case = bb.SIGMA6_CASE
    data, refs = setup(case)
    assert not np.array_equal(data.v, data.vh) and np.array_equal(bb.bf16_round(data.v), data.vh)
    assert np.array_equal(data.z, data.vh.astype(np.float64) @ data.O.astype(np.float64).T)
    x, y, _ = bb._link(case, data)
    ref = refs["exact"]
    gO = (x - y).T @ (float(bb.scale_of(case)) * data.v.astype(np.float64))
    dv = (x - y) @ data.O.astype(np.float64)
    # (float64 on both sides, the sums in another order: 1e-12 of the largest element covers the cancellation)
    assert ref["gO"] == pytest.approx(gO, rel=1e-12, abs=1e-12 * np.abs(gO).max())
    assert ref["dv"] == pytest.approx(dv, rel=1e-12, abs=1e-12 * np.abs(dv).max())
    rounded = (x - y).T @ (float(bb.scale_of(case)) * data.vh.astype(np.float64))
    assert np.abs(rounded - gO).max() > 1e-4 * np.abs(gO).max(), "the two forms of gO differ visibly"


def test_rows_from_stored_probabilities_hold_the_emulation_and_refuse_another_chain():
    """The emulated rows against the rows formed from the emulation's own fp32 probabilities (dz = dp = 0): inside;
    against the probabilities of the UNROUNDED v (another operand of the chain, family G): outside."""
    for case in (bb.SIGMA6_CASE, bb.S_CASES[0], bb.SHAPE_CASES[3]):
        data, _ = setup(case)
        for mode in bb.MODES:
            fast = mode == "fast"
            P32 = bs.logistic32(data.z.astype(np.float32), fast)
            rows, bound = bb.rows_from_probabilities(case, data, P32)
            got = bb.emul(case, data, fast, bb.ROUTES[0])[0]
            assert cc._ratio(np.abs(got - rows), bound) <= 1.0
            if case.family == "G":
                z_other = data.v.astype(np.float64) @ data.O.astype(np.float64).T
                other, bound = bb.rows_from_probabilities(case, data, bs.logistic32(z_other.astype(np.float32), fast))
                assert cc._ratio(np.abs(got - other), bound) > 1.0


# ------------------------------------------------------------------------------------- mutants fail -------
def _ratios(case, mutant, cuts=None):
    data, refs = setup(case)
    m = bb.reference(case, data, mutant, cuts)
    with np.errstate(invalid="ignore"):
        got = m["rows"], m["dv"].astype(np.float32), m["gO"].astype(np.float32)
    return [bb.verdict(refs[mode], *got) for mode in bb.MODES]


@pytest.mark.parametrize("mutant", [m for m in bb.MUTANTS if m not in bb.BLOCK_MUTANTS])
def test_mutant_fails(mutant):
    """Outside the bound under BOTH logistics' bounds (the exact one's is the tighter)."""
    failed = {}
    for case in bb.MUTANT_CASES:
        if mutant in ("sv_lo_dropped", "go_from_rounded_v") and case.family != "G":
            continue                                 # families E and S: no lo halves, v^ = v
        worst = np.min(np.array(_ratios(case, mutant)), axis=0)
        if worst.max() > 1.0:
            failed[case.name] = "rows dv gO".split()[int(np.argmax(worst))] + f" x{worst.max():.3g}"
    print(f"\n[bce stream bf16] mutant {mutant} fails {failed}")
    assert failed


@pytest.mark.parametrize("mutant", bb.BLOCK_MUTANTS)
def test_block_mutant_fails_by_a_factor_of_ten(mutant):
    part = bb.MUTANT_PART
    factor = np.min(np.array(_ratios(part.case, mutant, part.cuts)), axis=0).max() / 2.0       # the block form's allowance
    print(f"\n[bce stream bf16 part] mutant {mutant} leaves the doubled bound on {part.name} by a factor of {factor:.3g}")
    assert factor >= 10.0
    if mutant == "local_smoothing":
        assert bb.smoothing_miss_factor() == pytest.approx(factor)
    failed = [p.name for p in bb.PART_CASES[:3] if np.min(np.array(_ratios(p.case, mutant, p.cuts)), axis=0).max() > 2.0]
    print(f"[bce stream bf16 part] mutant {mutant} fails {failed}")
    assert failed


def test_the_dropped_mutant_is_the_identity_on_bf16_operands():
    """O_lo_dropped of bce_stream_cases: a bf16 O times a power of two is one fp16 value, there is no lo half to drop."""
    assert "O_lo_dropped" in bs.MUTANTS and "O_lo_dropped" not in bb.MUTANTS
    assert set(bb.MUTANTS) == (set(bs.MUTANTS) - {"O_lo_dropped"}) | set(bb.NEW_MUTANTS)
    for case in bb.MUTANT_CASES:
        data, _ = setup(case)
        a, b = bs.reference(case, data, "O_lo_dropped"), bs.reference(case, data)
        floor = 2.0 ** -38 * np.abs(data.O).max() * case.N
        assert np.abs(a["dv"] - b["dv"]).max() <= floor


# ------------------------------------------------------------------------------------- stated conditions --
@pytest.mark.parametrize("case", ALL_CASES, **by_name)
def test_operands_are_what_the_derivation_states(case):
    data, _ = setup(case)
    assert np.array_equal(bb.bf16_round(data.O), data.O), "O is exact in bf16"
    assert np.array_equal(bb.bf16_round(data.v), data.vh)
    dz = bb.chain_bound(case, data)
    if case.family in ("E", "S"):
        assert np.array_equal(data.v, data.vh)
        bb.assert_exact(case, data)
        assert not dz.any()
    else:
        low = np.ascontiguousarray(data.v).view(np.uint32) & 0xFFFF
        assert (low != 0).mean() > 0.99, "v has full mantissas"
        assert np.all(np.abs(data.z) + dz <= bs.Z_MAX)
        assert dz.max() > 0
    if case.family != "S":
        assert np.all(np.abs(data.z) + dz <= bs.Z_MAX)


def test_case_lists_cover_what_the_issue_names():
    assert sorted(c.ks for c in bb.KS_CASES) == [1, 2, 13, 16, 17, 32] and {(c.B, c.N) for c in bb.KS_CASES} == {(33, 97)}
    every = ALL_CASES
    assert {16, 24, 128, 136, 256, 264, 512} <= {c.c for c in every}
    assert {c.N for c in bb.CASES} == {97, 3003} and {c.B for c in bb.CASES} == {33, 70, 129}
    assert all(c.c % 8 == 0 and c.c <= 512 for c in every)
    assert [bb.chunk_columns(c) for c in (16, 128, 136, 256, 264, 512)] == [(1, 32), (1, 128), (2, 96), (2, 128), (3, 96), (4, 128)]
    assert all(c.lengths == cc.STREAM_LENGTHS for c in every)
    assert sum(c.sigma == 6.0 for c in bb.CASES) == 1 and sum(c.unit_scale for c in bb.CASES) == 1
    assert sum(c.eps == 0.0 for c in bb.CASES) == 2
    for c in (136, 512):
        cuts = [p.cuts for p in bb.PART_CASES if p.case.c == c and p.case.family == "G"]
        assert cuts == [(0, 1501, 3003), (0, 1000, 1001, 3003), (0, 2000, 3003), tuple(3003 * i // 8 for i in range(9))]
    part = bb.MUTANT_PART
    assert (part.case.N, part.cuts, part.case.eps) == (64, (0, 32, 64), 0.5)
    # every new mutant has a case on which it is not the identity: more than one chunk among the mutants' cases
    assert any(bb.chunk_columns(c.c)[0] > 1 for c in bb.MUTANT_CASES)
