"""The cases of tests/golden/cand_cases.py, proved on the host (numpy only, no GPU).

  * the method: every product v o / dz o is a float32 number, so the emulations' float32 adds are the kernels' fmaf;
    the forward's emulation agrees with float64 within gamma(m + 6) sum |v^||o|, the dv emulation within
    gamma(ceil(K / 4) + 2) sum |dz o| per element;
  * the 64 lanes of the butterfly end with the same bits;
  * coverage: the union of features() over the case list equals the label set;
  * mutants: each other order of the forward (sequential lane sum, butterfly the other way, lane-contiguous elements,
    chunks descending; for bf16 a truncated or half-away v) and of dv (floor(K / 4), decreasing k, one chain, pairwise
    combine, invalid ids added) changes the bits of at least one case of its kernel and type.
A mutant that changes nothing means the cases are too tame: the cases are changed, not the mutant.
"""
import numpy as np
import pytest

import cand_cases as cc

CASES = cc.CASES
by_name = dict(ids=lambda c: c.name)
SMALL = 200_000                     # entries x rank up to which the mutants are run


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Equal bits, NaN entries equal to NaN entries whatever their payload."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def test_names_are_unique_and_every_case_is_small():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES:
        assert 1 <= c.c <= cc.MAXC and c.n_ent * c.c * 4 <= 2 << 20 and c.B * c.K * c.c <= 650_000, c.name
        assert c.B * c.K <= 4096 or c.c == 4, f"{c.name}: a case about batch x K keeps c = 4"
        assert set(c.kernels) <= {"fwd", "dv"} and c.kernels
    for bf16, name in cc.BOTH_OUTPUTS.items():
        case = cc.BY_NAME[name]
        assert case.bf16 == bf16 and not case.bad and case.kernels == ("fwd", "dv")


def test_coverage_equals_the_label_set():
    reached = set()
    for c in CASES:
        reached |= cc.features(c)
    assert reached == cc.LABELS, (sorted(cc.LABELS - reached), sorted(reached - cc.LABELS))


def test_quarter_rule():
    table = {1: [(0, 1), (1, 1), (1, 1), (1, 1)], 2: [(0, 1), (1, 2), (2, 2), (2, 2)],
             3: [(0, 1), (1, 2), (2, 3), (3, 3)], 4: [(0, 1), (1, 2), (2, 3), (3, 4)],
             5: [(0, 2), (2, 4), (4, 5), (5, 5)], 6: [(0, 2), (2, 4), (4, 6), (6, 6)],
             7: [(0, 2), (2, 4), (4, 6), (6, 7)], 8: [(0, 2), (2, 4), (4, 6), (6, 8)],
             9: [(0, 3), (3, 6), (6, 9), (9, 9)], 33: [(0, 9), (9, 18), (18, 27), (27, 33)]}
    for K, want in table.items():
        assert cc.quarters(K) == want, K
    assert cc.quarters(0) == [(0, 0)] * 4
    assert cc.quarters(5, floor=True) == [(0, 1), (1, 2), (2, 3), (3, 5)]
    assert cc.quarters(3, floor=True) == [(0, 0), (0, 0), (0, 0), (0, 3)]


def test_span_rule():
    assert cc.span_of(3, 50001) == (16, 3126) and 50001 - 3125 * 16 == 1
    assert cc.span_of(5, 7) == (7, 1) and cc.span_of(4096, 1000) == (256, 4) and cc.span_of(1, 1) == (1, 1)
    assert cc.span_of(16384, 8) == (8, 1) and cc.span_of(16385, 16) == (16, 1) and cc.span_of(8192, 17) == (16, 2)


def test_bf16_roundings():
    x = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000], dtype=np.uint32).view(np.float32)
    assert bits(cc.bf16_rne(x)).tolist() == [0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0xBF800000, 0xBF820000]
    assert bits(cc.bf16_trunc(x)).tolist() == [0x3F800000, 0x3F810000, 0x3F800000, 0x3F800000, 0xBF800000, 0xBF810000]
    assert bits(cc.bf16_half_up(x)).tolist() == [0x3F810000, 0x3F820000, 0x3F810000, 0x3F800000, 0xBF810000, 0xBF820000]


@pytest.mark.parametrize("case", CASES, **by_name)
def test_operands_are_narrow_and_products_exact(case):
    op = cc.operands(case)
    B, K, c = case.B, case.K, case.c
    ids, ok = cc.ids_of(case)
    assert op.cand.shape == (1 if case.shared else B, K + case.cand_pad) and op.cand.dtype == np.int64
    assert (op.cand[:, K:] == 0).all() and np.all(op.dz[:, K:] == cc.SENTINEL)
    g = op.dz[:, :K]
    assert op.dz.dtype == op.v.dtype == op.O.dtype == np.float32
    assert np.array_equal(cc.round_mantissa(g[ok], 12), g[ok]) and not np.isfinite(g[~ok]).any()
    assert np.array_equal(cc.round_mantissa(op.v, 12), op.v)
    assert np.array_equal(cc.round_mantissa(op.O, 8 if case.bf16 else 12), op.O)
    if case.bf16:
        assert not (bits(op.O) & 0xFFFF).any(), "O does not hold bf16 values"
        vh = cc.forward_v(case)
        assert not (bits(vh) & 0xFFFF).any() and (vh != op.v).any() == (op.v.size > 0)
        assert (np.abs(vh.astype(np.float64) - op.v) <= np.abs(op.v) * 2.0 ** -8).all()
    assert (~ok).sum() == len(case.bad) * B and cc.expected_error_word(case) == (2 if case.bad and B * K else 0)
    if B * K:                                           # sampled products, computed in float64: float32 holds them
        e = np.clip(ids[:, 0], 0, case.n_ent - 1)
        for a, b in ((cc.forward_v(case), op.O[e]), (np.where(ok[:, :1], g[:, :1], 1).astype(np.float32), op.O[e])):
            p32 = a * b
            assert p32.dtype == np.float32 and np.array_equal(p32.astype(np.float64), a.astype(np.float64) * b)


@pytest.mark.parametrize("case", cc.cases_of("fwd"), **by_name)
def test_forward_emulation_within_the_float64_bound_and_lanes_agree(case):
    z64, bound = cc.reference_fwd(case)
    lanes = cc.forward_lanes(case)
    assert lanes.dtype == np.float32 and lanes.shape == (case.B * case.K, cc.LANES)
    assert (bits(lanes) == bits(lanes[:, :1])).all(), "the 64 lanes of the butterfly end with different bits"
    got = cc.expected_fwd(case)
    _, ok = cc.ids_of(case)
    assert got.shape == (case.B, case.K) and np.array_equal(np.isnan(got), ~ok)
    err = np.abs(got.astype(np.float64) - z64)[ok]
    assert (err <= bound[ok]).all(), f"max excess {(err - bound[ok]).max():.3e}"
    if case.B * case.K and case.c >= 3:
        assert (err > 0).any(), "nothing rounds: the exponents are too tame"


@pytest.mark.parametrize("case", cc.cases_of("dv"), **by_name)
def test_dv_emulation_within_the_float64_bound(case):
    g64, bound = cc.reference_dv(case)
    got = cc.expected_dv(case)
    assert got.dtype == np.float32 and got.shape == (case.B, case.c) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - g64)
    assert (err <= bound).all(), f"max excess {(err - bound).max():.3e}"
    if case.K == 0:
        assert not bits(got).any(), "dv of an empty list is not +0"
    if case.B and case.K >= 3:
        assert (err > 0).any(), "nothing rounds: the exponents are too tame"


def _seen_by(mutant, cases, expected):
    return [c.name for c in cases if c.B * c.K and c.B * c.K * c.c <= SMALL and not same(mutant(c), expected(c))]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant", sorted(cc.FWD_MUTANTS))
def test_each_forward_mutant_changes_the_bits_of_some_case(mutant, bf16):
    seen = _seen_by(cc.FWD_MUTANTS[mutant], cc.cases_of("fwd", bf16), cc.expected_fwd)
    print(f"\n[forward, {'bf16' if bf16 else 'f32'}: {mutant}] changes {len(seen)} cases: {', '.join(seen)}")
    assert seen, f"no case sees the mutant '{mutant}'"


@pytest.mark.parametrize("mutant", sorted(cc.FWD_MUTANTS_BF16))
def test_each_v_rounding_mutant_changes_the_bits_of_some_case(mutant):
    cases = cc.cases_of("fwd", True)
    seen = _seen_by(cc.FWD_MUTANTS_BF16[mutant], cases, cc.expected_fwd)
    print(f"\n[forward, bf16: {mutant}] changes {len(seen)} cases: {', '.join(seen)}")
    assert seen, f"no case sees the mutant '{mutant}'"
    assert all("v_rne_tie" in cc.features(c) for c in cases if c.B * c.K and c.B * c.c >= 4), \
        "a bf16 case without halfway values of both parities in v"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant", sorted(cc.DV_MUTANTS))
def test_each_dv_mutant_changes_the_bits_of_some_case(mutant, bf16):
    seen = _seen_by(cc.DV_MUTANTS[mutant], cc.cases_of("dv", bf16), cc.expected_dv)
    print(f"\n[dv, {'bf16' if bf16 else 'f32'}: {mutant}] changes {len(seen)} cases: {', '.join(seen)}")
    assert seen, f"no case sees the mutant '{mutant}'"


def test_the_mutants_are_seen_where_they_are_meant_to_be():
    """floor(K / 4) is the same rule at K = 4 n and another one everywhere else; the chunk order needs two chunks."""
    floor = cc.DV_MUTANTS["quarter = floor(K / 4)"]
    for case in cc.cases_of("dv"):
        if case.B and case.K >= 5:
            assert same(floor(case), cc.expected_dv(case)) == (case.K % 4 == 0), case.name
    desc = cc.FWD_MUTANTS["chunks in descending order"]
    for case in cc.cases_of("fwd"):
        if case.B * case.K and case.B * case.K * case.c <= SMALL:
            assert same(desc(case), cc.expected_fwd(case)) or case.nch >= 2, case.name
