"""The cases of tests/golden/chol_cases.py, proved on the host (numpy only, no GPU).

  * coverage: the union of features() over the case list equals the label set;
  * the references stay inside every cap: the unblocked sweep in float64 and the blocked float64 model both pass the
    checks the device has to pass (B1 - B4, the floor path's figures, the zero column), measured against the
    extended-precision sweep; the model and the unblocked float64 sweep do not share a summation order, so the caps
    are not fitted to one order;
  * the floored sets are what the case list says, and no pivot of a floor case is near its floor;
  * mutants of the model each break at least one check on at least one case.
A mutant that survives means the cases are changed, not the mutant.
"""
import numpy as np
import pytest

import chol_cases as cc

by_name = dict(ids=lambda c: c.name)
U = cc.U


def test_names_are_unique_and_every_case_is_small():
    names = [c.name for c in cc.CASES]
    assert len(names) == len(set(names))
    assert all(1 <= c.k <= cc.KMAX for c in cc.CASES)
    assert {c.k for c in cc.GRID} == set(cc.SIZES) and len(cc.GRID) == len(cc.SIZES) * len(cc.FAMILIES) * len(cc.MODES)


def test_coverage_equals_the_label_set():
    reached = set()
    for c in cc.CASES:
        reached |= cc.features(c)
    assert reached == cc.LABELS, (sorted(cc.LABELS - reached), sorted(reached - cc.LABELS))
    # the sizes the issue names, by the branch they are there for
    f = {k: cc.features(cc.BY_NAME[f"plain-k{k}-m0"]) for k in cc.SIZES}
    assert "only_block_partial" in f[15] and "only_block_full" in f[32] and "k1" in f[1]
    assert "below_15" in f[47] and "below_16" in f[48] and "below_17" in f[49] and "below_0" in f[64]
    assert {"nlt_max", "nbt_max", "ntri_above_waves"} <= f[255] and {"nlt_max", "nbt_max"} <= f[256]
    assert "ntri_below_waves" in f[96] and "copyin_last_full" in f[256] and "copyin_last_partial" in f[255]


def test_the_extended_precision_is_extended():
    assert cc.EXTENDED in ("longdouble", "mpmath")
    if cc.EXTENDED == "longdouble":
        assert np.finfo(np.longdouble).eps < 1e-18


def test_the_mpmath_sweep_agrees_with_the_extended_one():
    """The fallback of a platform whose longdouble is a double is the same algorithm: at k = 6 it agrees with the
    extended sweep to the extended precision, and it floors the same column."""
    case = cc.CholCase("dup-k6", "plain", 6, cc.MODES[0], kind="dup", col=3, floored=(3,))
    S = cc.matrix(case)
    R, X, fl = cc.truth(S, *case.mode)
    Rm, Xm, flm = cc.truth(S, *case.mode, hp="mpmath")
    assert fl == flm == [3]
    lead = (slice(0, 3), slice(0, 3))                   # behind the floored pivot: rounding noise over sqrt(floor)
    assert cc.forward_error(cc._f64(Rm)[lead], R[lead]) < 4 * U and cc.forward_error(cc._f64(Xm)[lead], X[lead]) < 4 * U
    rho = cc.residuals(S[:3, :3], cc._f64(Rm)[lead], cc._f64(Xm)[lead], *case.mode, hp="mpmath")
    assert max(rho.values()) < 4 * U


@pytest.mark.parametrize("case", cc.GRID + cc.ZEROCOL, **by_name)
def test_float64_sweep_and_model_stay_inside_the_caps(case):
    ref = cc.reference(case)
    assert ref.floored == list(case.floored) == [] and ref.model[2] == []
    bad, _ = cc.check(case, ref.model[0], ref.model[1], rho=ref.model_rho)
    assert not bad, f"[{case.name}] model64: " + "; ".join(bad)
    R64, X64, fl = cc.truth(cc.matrix(case), *case.mode, hp="float64")
    assert fl == []
    bad, _ = cc.check(case, R64, X64)
    assert not bad, f"[{case.name}] float64 sweep: " + "; ".join(bad)


@pytest.mark.parametrize("case", cc.FLOOR, **by_name)
def test_floor_cases_floor_what_the_list_says_decisively(case):
    ref = cc.reference(case)
    assert ref.floored == list(case.floored) and ref.model[2] == list(case.floored) and case.floored
    # no near-tie decides a branch: every pivot of the extended sweep is at least 5 % away from its floor
    S = cc.matrix(case)
    sc = cc.scaled(S, *case.mode)
    L = (ref.R / sc.D[None, :]).T
    raw = cc._f64((sc.A.diagonal() - (np.tril(L, -1) ** 2).sum(1)) / sc.floor)      # pivots before flooring / floor
    floored = np.zeros(case.k, dtype=bool)
    floored[list(case.floored)] = True
    assert (raw[~floored] > 1.05).all() and (raw[floored] < 0.95).all(), (raw[~floored].min(), raw[floored].max())
    if case.kind == "dup":                              # the cancelled pivot is rounding noise, orders below its floor
        assert abs(raw[case.col]) < 1e-3, raw[case.col]
    for who, (R, X) in (("model64", ref.model[:2]), ("float64 sweep", cc.truth(S, *case.mode, hp="float64")[:2])):
        bad, fig = cc.check(case, R, X)
        assert not bad, f"[{case.name}] {who}: " + "; ".join(bad)
        assert {"lead_R", "lead_X", "max_X"} <= set(fig) and all(f"pivot_{c}" in fig for c in case.floored)


def test_the_f32_gram_case_is_inside_the_contract():
    """Positive semi-definite plus noise: the float64 Gram matrix of the same columns is positive semi-definite, and the
    case differs from it by float32 rounding noise of about one shift on the equilibrated scale."""
    case = cc.BY_NAME["f32gram-k60"]
    S, W = cc.matrix(case), cc.factor(case)
    exact = W.T @ W
    d = np.sqrt(exact.diagonal())
    noise = np.abs(S - exact) / np.outer(d, d)
    assert 1e-7 < noise.max() < 2 * case.mode[1], noise.max()
    sv = np.linalg.svd(W / d, compute_uv=False)          # 20 of the 60 columns are dependent to float32 rounding
    assert sv[39] > 1e-2 * sv[0] and sv[40] < 1e-6 * sv[0], (sv[39] / sv[0], sv[40] / sv[0])
    assert np.linalg.eigvalsh(exact / np.outer(d, d)).min() > -1e-12


@pytest.mark.parametrize("case", cc.PLANTED, **by_name)
def test_non_finite_contract_of_the_references(case):
    """On or below the diagonal: zero outputs.  Above: never read."""
    S = cc.matrix(case)
    i, j = case.at
    for R, X, fl in (cc.truth(S, *case.mode), cc.model64(S, *case.mode)):
        R, X = cc._f64(R), cc._f64(X)
        if i >= j:
            assert not R.view(np.uint64).any() and not X.view(np.uint64).any() and fl == []
            assert cc.check(case, R, X) == ([], {})
        else:
            assert np.isfinite(R).all() and np.isfinite(X).all() and R.any()
    if i < j:
        Rc, Xc, _ = cc.model64(cc.matrix(cc.clean(case)), *case.mode)
        R, X, _ = cc.model64(S, *case.mode)
        assert np.array_equal(R.view(np.uint64), Rc.view(np.uint64)) and np.array_equal(X.view(np.uint64), Xc.view(np.uint64))


def test_zero_and_negative_trace_give_zero():
    for S in (np.zeros((9, 9)), -np.eye(4)):
        for R, X, fl in (cc.truth(S, 1, 1e-13, 0.0), cc.model64(S, 1, 1e-13, 0.0)):
            assert not cc._f64(R).any() and not cc._f64(X).any() and fl == []


# the cases a mutant is tried on: every branch of the sweep at the small sizes, the floor path, the zero columns
MUTANT_CASES = tuple(c for c in cc.CASES if c.kind != "plant" and c.k <= 65)


@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_each_mutant_breaks_a_check_on_some_case(mutant):
    seen = []
    for case in MUTANT_CASES:
        with np.errstate(all="ignore"):
            R, X, _ = cc.model64(cc.matrix(case), *case.mode, mutant=mutant)
            bad, _ = cc.check(case, R, X)
        if bad:
            seen.append(f"{case.name} ({bad[0]})")
    print(f"\n[{mutant}] breaks {len(seen)} of {len(MUTANT_CASES)} cases; first: {seen[:3]}")
    assert seen, f"no case sees the mutant '{mutant}'"


def test_each_mutant_is_seen_where_it_is_meant_to_be():
    """The mutants are about one branch each: the case that is there for that branch sees it."""
    want = dict(newton="plain-k1-m0", tile_skip="plain-k47-m0", left_minus_1="plain-k33-m1", d_wrong_side="scaled-k17-m1",
                unzeroed="plain-k2-m0", floor_rel_only="f32gram-k60")
    assert set(want) == set(cc.MUTANTS)
    for mutant, name in want.items():
        case = cc.BY_NAME[name]
        with np.errstate(all="ignore"):
            R, X, _ = cc.model64(cc.matrix(case), *case.mode, mutant=mutant)
            bad, _ = cc.check(case, R, X)
        assert bad, f"{name} does not see '{mutant}'"
