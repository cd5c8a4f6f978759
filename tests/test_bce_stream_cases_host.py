"""The method of tests/test_gpu_bce_stream_kernels.py, proved without a GPU on the cases of
tests/golden/bce_stream_cases.py:

  * the fp32 numpy emulation of the BCE link (both logistics, rtk_clog, the sixteen fp32 adds per lane and tile, the
    hi/lo split of x and the two tile products) stays within the derived bounds of rows, dv and gO on every case, also
    with every exponential moved one ulp up or down;
  * every named mutant -- a kernel that is wrong in one way -- is outside its bound on at least one case, judged by
    the verdict function the GPU test uses; the two block mutants leave the doubled bound of the block form by a factor
    of ten or more on the n_ent = 64 case;
  * the conditions the derivation states hold: no logit where saturation is ambiguous, exact logits in families E
    and S, every planted level on a listed positive and on a negative, the CSR's conventions.
"""
import functools

import numpy as np
import pytest

import bce_stream_cases as bs
import ce_kernel_cases as cc

by_name = dict(ids=lambda c: c.name)
ALL_CASES = bs.CASES + [bs.MUTANT_PART.case] + sorted({p.case for p in bs.PART_CASES} - set(bs.CASES), key=lambda c: c.name)


@functools.lru_cache(maxsize=None)
def setup(case):
    data = bs.operands(case)
    bs.assert_unambiguous(case, data)               # before anything is judged (and before anything goes to a GPU)
    return data, {mode: bs.bounds(case, data, mode == "fast") for mode in bs.MODES}


# ------------------------------------------------------------------------------------- emulations pass ----
@pytest.mark.parametrize("case", ALL_CASES, **by_name)
def test_emulation_within_bounds(case):
    data, refs = setup(case)
    for mode in bs.MODES:
        for perturb in (0, 1, -1):
            r = bs.verdict(refs[mode], *bs.emul(case, data, mode == "fast", perturb))
            print(f"\n[bce stream, emulated] {case.name} {mode} {perturb:+d}: error / bound = {r[0]:.4f} (rows), "
                  f"{r[1]:.4f} (dv), {r[2]:.4f} (gO)")
            assert max(r) <= 1.0


def test_the_float64_reference_passes_its_own_verdict():
    for case in (bs.S_CASES[0], bs.SIGMA6_CASE):
        data, refs = setup(case)
        ref = refs["fast"]
        assert max(bs.verdict(ref, ref["rows"], ref["dv"].astype(np.float32), ref["gO"].astype(np.float32))) <= 1.0
        assert bs.reference(case, data, cuts=(0, 40, case.N))["rows"] == pytest.approx(ref["rows"], rel=1e-13)


# ------------------------------------------------------------------------------------- mutants fail -------
def _ratios(case, mutant, cuts=None):
    data, refs = setup(case)
    m = bs.reference(case, data, mutant, cuts)
    with np.errstate(invalid="ignore"):
        got = m["rows"], m["dv"].astype(np.float32), m["gO"].astype(np.float32)
    return [bs.verdict(refs[mode], *got) for mode in bs.MODES]


@pytest.mark.parametrize("mutant", [m for m in bs.MUTANTS if m not in bs.BLOCK_MUTANTS])
def test_mutant_fails(mutant):
    """Outside the bound under BOTH logistics' bounds (the exact one's is the tighter)."""
    failed = {}
    for case in bs.MUTANT_CASES:
        if mutant in ("O_lo_dropped", "sv_lo_dropped") and case.family != "G":
            continue                                 # families E and S have no lo halves
        worst = np.min(np.array(_ratios(case, mutant)), axis=0)
        if worst.max() > 1.0:
            failed[case.name] = "rows dv gO".split()[int(np.argmax(worst))] + f" x{worst.max():.3g}"
    print(f"\n[bce stream] mutant {mutant} fails {failed}")
    assert failed


@pytest.mark.parametrize("mutant", bs.BLOCK_MUTANTS)
def test_block_mutant_fails_by_a_factor_of_ten(mutant):
    part = bs.MUTANT_PART
    factor = np.min(np.array(_ratios(part.case, mutant, part.cuts)), axis=0).max() / 2.0       # the block form's allowance
    print(f"\n[bce stream part] mutant {mutant} leaves the doubled bound on {part.name} by a factor of {factor:.3g}")
    assert factor >= 10.0
    if mutant == "local_smoothing":
        assert bs.smoothing_miss_factor() == pytest.approx(factor)
    failed = [p.name for p in bs.PART_CASES[:3] if np.min(np.array(_ratios(p.case, mutant, p.cuts)), axis=0).max() > 2.0]
    print(f"[bce stream part] mutant {mutant} fails {failed}")
    assert failed


def test_a_nonzero_bit_in_a_quiet_row_is_refused():
    case = bs.S_CASES[0]
    _, refs = setup(case)
    ref = refs["exact"]
    assert ref["quiet_q"].sum() >= 6 and ref["quiet_e"].sum() == 2
    rows, dv, gO = ref["rows"], ref["dv"].astype(np.float32), ref["gO"].astype(np.float32)
    assert max(bs.verdict(ref, rows, dv, gO)) <= 1.0
    bad = dv.copy()
    bad[np.nonzero(ref["quiet_q"])[0][0], 3] = np.float32(-0.0)
    assert bs.verdict(ref, rows, bad, gO)[1] == np.inf
    bad = gO.copy()
    bad[np.nonzero(ref["quiet_e"])[0][1], 0] = np.float32(-0.0)
    assert bs.verdict(ref, rows, dv, bad)[2] == np.inf


# ------------------------------------------------------------------------------------- stated conditions --
@pytest.mark.parametrize("case", ALL_CASES, **by_name)
def test_no_ambiguous_element_and_exact_families(case):
    data, _ = setup(case)
    bs.assert_unambiguous(case, data)
    if case.family in ("E", "S"):
        bs.assert_exact(case, data)
        assert not bs.chain_bound(case, data).any()
    else:
        assert np.abs(data.z).max() <= 14.5 + 1e-5


def test_family_s_plants_every_level_on_positives_and_negatives():
    for case in bs.S_CASES:
        data, refs = setup(case)
        z, P = data.z, bs.positives_mask(case, data.csr)
        s1, s0 = bs.saturated(z)
        assert z[s1].min() >= 17.0 and z[s0].max() <= -104.0
        for j in bs.plant_columns(case.N):
            for sat in (s1, s0):
                assert (sat[:, j] & P[:, j]).any() and (sat[:, j] & ~P[:, j]).any(), (case.name, j)
        quiet = np.nonzero(refs["exact"]["quiet_q"])[0]
        assert len(quiet) >= case.B // 5 and any(P[d].any() for d in quiet), "an all-saturated row with a list"
        assert (data.csr.slot == -1).sum() == 1 and list(np.nonzero(refs["exact"]["quiet_e"])[0]) == bs.dead_columns(case.N)
        assert P[:, bs.dead_columns(case.N)].any(), "a listed positive on a column that saturates for every query"
        live = ~(s1 | s0)
        assert live.mean() > 0.6 and 1.5 <= z[live].std() <= 3.5


def test_csr_conventions():
    for case in ALL_CASES:
        csr = setup(case)[0].csr
        top = case.below or case.N
        for s, n in enumerate(case.lengths):
            l = csr.obj[csr.ptr[s]:csr.ptr[s + 1]]
            if n >= 6:
                assert {-1, case.N, case.N + 5} <= set(l.tolist())
            good = l[(l >= 0) & (l < case.N)]
            assert len(set(good.tolist())) == len(good), "no object twice in a list (the header's precondition)"
            assert good.max(initial=0) < top
            if len(good) >= 2 and case.N >= 4:
                assert {0, top - 1} <= set(good.tolist())
        if case.B >= 31:
            assert (csr.slot == -1).sum() == 1 and csr.slot[case.B - 1] == 0 and case.lengths == cc.STREAM_LENGTHS


def test_case_lists_cover_what_the_issue_names():
    assert sorted(c.c // 16 for c in bs.KS_CASES) == list(range(1, 14)) and {(c.B, c.N) for c in bs.KS_CASES} == {(33, 97)}
    assert {(c.B, c.N, c.c) for c in bs.SHAPE_CASES} == {(1, 1, 4), (31, 33, 16), (33, 95, 20), (32, 3003, 36),
                                                        (129, 3003, 64), (513, 257, 32), (70, 4099, 100), (70, 3003, 208)}
    assert all({c.family for c in bs.SHAPE_CASES if c.B == B} == {"E", "G"} for B in (1, 31, 513))
    assert sum(c.eps == 0.0 for c in bs.CASES) == 2 and all(c.eps in (0.0, 0.1) for c in bs.CASES)
    assert [(c.B, c.N, c.c) for c in bs.S_CASES] == [(33, 97, 16), (70, 3003, 36), (70, 3003, 208)]
    assert sum(c.sigma == 6.0 for c in bs.CASES) == 1 and sum(c.unit_scale for c in bs.CASES) == 1
    assert cc.splits_of(513) == 51
    s = float(bs.scale_of(bs.SHAPE_CASES[-1]))
    assert s == pytest.approx(-3.0 / (70 * 3003)) and abs(np.log2(abs(s))) > 15
    assert float(bs.scale_of(bs.UNIT_SCALE_CASE)) == 1.0
    for c in (36, 208):
        cuts = [p.cuts for p in bs.PART_CASES if p.case.c == c and p.case.family == "G"]
        assert cuts == [(0, 1501, 3003), (0, 1000, 1001, 3003), (0, 2000, 3003), tuple(3003 * i // 8 for i in range(9))]
    assert 1501 % 32 and len(bs.PART_CASES[3].blocks) == 8
    part = bs.MUTANT_PART
    assert (part.case.N, part.cuts, part.case.eps) == (64, (0, 32, 64), 0.5)
