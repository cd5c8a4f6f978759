"""Host checks of tests/golden/sf16_gemm_cases.py, the numpy model of rtk_gemm_sf16_splitk and the operands on which it is
exact (no GPU): the shift rule, the exactness criterion of every case (headroom printed per family), fp32 accumulation
of the products per chunk in random orders followed by the fp32 slab adds, and the mutants (each must change outputs of
an exact case on every shape it applies to; the share on the worst shape is printed)."""
import numpy as np
import pytest

import sf16_gemm_cases as gc

F32, F64 = np.float32, np.float64
_cache = {}
_head = {}
_share = {}


def case_of(shape, family):
    key = (shape.id, family)
    if key not in _cache:
        _cache[key] = gc.make_case(shape, family)
    return _cache[key]


def all_cases():
    for shape in gc.SHAPES:
        for family in gc.FAMILIES_ALL_SHAPES:
            yield case_of(shape, family)
    yield case_of(gc.LONG, "hionly")
    for shape in (gc.SMALL, gc.SMALL_SPLIT):
        for family in gc.small_families():
            case = case_of(shape, family)
            if case is not None:
                yield case
    for family in gc.pos_families():
        case = case_of(gc.POS_SHAPE, family)
        if case is not None:
            yield case
    for v in ("ratio3", "ratio1024"):
        yield case_of(gc.CONTROL, f"bound:{v}:A")


def test_operand_shift_rule():
    f = lambda x: int(gc.operand_shift(np.array([x], dtype=F32))[0])
    assert [f(16384.0), f(32767.0), f(32768.0), f(1.0), f(0.75), f(-3.0), f(2.0 ** -80)] == [0, 0, -1, 14, 15, 13, 94]
    assert f(2.0 ** -86) == 100 and f(2.0 ** -87) == 100 and f(2.0 ** -126) == 100          # the upper clamp
    assert f(2.0 ** -127) == 0 and f(2.0 ** -149) == 0 and f(0.0) == 0                      # zero, subnormal: scale 1
    assert int(gc.sc.pack_shift(F32(2.0 ** -127))) == 100                                   # (rtk_pack_shift differs)
    assert f(np.inf) == 0 and f(np.nan) == 0 and f(-np.inf) == 0
    assert f(2.0 ** 114) == -100 and f(2.0 ** 116) == -102 and f(3.4e38) == -113            # no lower clamp
    for e in range(-113, 101):      # both of an operand's factors are fp32 normals
        assert np.isfinite(F32(2.0) ** F32(e)) and F32(2.0) ** F32(e) >= F32(2.0 ** -126)
        assert np.isfinite(F32(2.0) ** F32(-e)) and F32(2.0) ** F32(-e) >= F32(2.0 ** -126)
    # the epilogue's factors: one whenever 2^s is a normal, else two normals of the same sign
    for ea in range(-113, 101, 3):
        for eb in range(-113, 101, 7):
            u1, u2 = gc.factors(ea, eb)
            s = -(ea + eb)
            assert float(u1) * float(u2) == 2.0 ** s and min(u1, u2) >= F32(2.0 ** -126) and np.isfinite([u1, u2]).all()
            assert (u2 == 1) == (-126 <= s <= 127) and (u1 > 1) == (u2 > 1) or u2 == 1
    assert gc.chunks(65, 4) == [(0, 32), (32, 64), (64, 65), (65, 65)] and gc.chunks(97, 3) == [(0, 64), (64, 97), (97, 97)]
    assert gc.chunks(20011, 7)[-1] == (17280, 20011) and gc.chunks(64, 2) == [(0, 32), (32, 64)] and gc.chunks(33, 1) == [(0, 33)]


def test_shapes_cover_the_branches():
    S = gc.SHAPES
    assert {s.K for s in S if s.splits == 1 and s.mode == "vec"} >= set(gc.K_SWEEP)
    assert {s.mode for s in S} == {"vec", "off", "odd"}
    assert {s.M for s in S} >= {1, 31, 32, 33, 64, 65, 127, 128, 129, 257} <= {s.N for s in S}
    assert {s.tiles for s in S} >= {1, 3, 6, 8, 9, 17, 18}
    assert {s.splits for s in S} | {gc.LONG.splits} >= {1, 2, 3, 4, 7}
    assert any(s.splits > 1 and gc.chunks(s.K, s.splits)[-1][0] == s.K for s in S)                 # a chunk past K
    assert any(s.splits > 1 and len({b - a for a, b in gc.chunks(s.K, s.splits)}) == 1 for s in S)   # equal chunks
    assert any(s.splits > 1 and (s.M * s.N * 4) % 256 for s in S) and any(s.splits > -(-s.K // 32) for s in S)
    assert any(s.ldc_pad and s.c_off and s.splits == 1 for s in S)
    for s in S:
        for km, length in ((1, s.K), (0, s.M), (0, s.N)):
            pad, off = s.pad_off(km, length)
            assert pad > 0 and (not km or ((length + pad) % 4 == 0) == (s.mode != "odd")) and off == (km and s.mode == "off")
    for K in gc.K_SWEEP:
        pos = gc.tail_positions(K)
        assert pos[:2] == [K - 1, 0] and (len(pos) == 2) == (K <= 8) and all(p % 16 >= 8 and K - 17 <= p < K for p in pos[2:])


@pytest.mark.parametrize("shape", gc.SHAPES + [gc.LONG], ids=gc.SHAPE_IDS + [gc.LONG.id])
def test_exact_cases_hold_and_catch_the_mutants(shape):
    families = gc.FAMILIES_ALL_SHAPES if shape is not gc.LONG else ("hionly",)
    for family in families:
        check_case(case_of(shape, family))


@pytest.mark.parametrize("shape", [gc.SMALL, gc.SMALL_SPLIT, gc.CONTROL], ids=lambda s: s.id)
def test_bound_and_scale_cases_hold_and_catch_the_mutants(shape):
    if shape is gc.CONTROL:
        for v in ("ratio3", "ratio1024"):
            check_case(case_of(shape, f"bound:{v}:A"))
        return
    kept = set()
    for family in gc.small_families():
        case = case_of(shape, family)
        if case is None:
            continue
        check_case(case)
        if family.startswith("scale"):
            kept.add(tuple(int(x) for x in family.split(":")[1:]))
    print(f"{shape.id}: scale pairs kept: {len(kept)} of {len(gc.SCALE_EXPS) ** 2}")
    # the findings' pairs are there: 2^110 x 2^-60 (the first unscale step alone would overflow), a bound past 2^115,
    # a clamped shift (2^-120), and a pair whose 2^-(ea + eb) = 2^-128 is no fp32 normal
    assert {(110, -60), (-60, 110), (125, -60), (-120, 110), (-40, -60), (60, 60)} <= kept
    assert (110, 40) not in kept and (-120, 0) not in kept and (-60, -60) not in kept


def test_positive_scale_cases_hold():
    kept = set()
    for family in gc.pos_families():
        case = case_of(gc.POS_SHAPE, family)
        if case is not None:
            check_case(case)
            kept.add(tuple(int(x) for x in family.split(":")[1:]))
    print(f"positive scale pairs kept: {len(kept)}")
    assert {(110, -60), (-60, 110), (125, -60), (125, -120), (-40, -60), (0, 0)} <= kept
    # the first of the two separate factors 2^-ea, 2^-eb overflows on such an accumulator; the epilogue's do not
    m = case_of(gc.POS_SHAPE, "scalepos:110:-60").model
    with np.errstate(over="ignore"):
        assert np.abs(m.acc).min() >= 2.0 ** 32 and not np.isfinite(gc.unscale32(m.acc, (F32(2.0 ** -m.ea), F32(2.0 ** -m.eb)))).any() and np.isfinite(m.C).all()


def check_case(case):
    head = gc.assert_exact(case)
    kind = case.family.split(":")[0]
    _head[kind] = max(_head.get(kind, 0.0), head)
    m, P, ok, shape = case.model, case.P, case.valid, case.shape
    rng = np.random.default_rng(5)
    # fp32 accumulation of the products, per chunk, three random orders, then the fp32 slab adds in chunk order
    ii, jj = np.nonzero(ok)
    pick = rng.choice(ii.size, size=min(24, ii.size), replace=False)
    u = gc.factors(m.ea, m.eb)
    for i, j in zip(ii[pick], jj[pick]):
        for _ in range(3):
            slabs = []
            for k0, k1 in gc.chunks(shape.K, shape.splits):
                sl = slice(k0, k1)
                prods = np.concatenate([P.vh[i, sl] * P.oh[j, sl], P.vh[i, sl] * P.ol[j, sl], P.vl[i, sl] * P.oh[j, sl]])
                p32 = prods.astype(F32)
                assert np.array_equal(p32.astype(F64), prods)
                s = np.cumsum(rng.permutation(p32), dtype=F32)[-1] if p32.size else F32(0)
                slabs.append(gc.unscale32(np.asarray(s, dtype=F64), u))
            c = gc.reduce32(slabs)
            assert c == m.C[i, j] and F64(c) == m.C64[i, j], (case.name, i, j)
    nz = m.C[ok][m.C[ok] != 0]
    print(f"{case.name}: max T / g = 2^{np.log2(max(head, 1.0)):.2f}; shifts {m.ea}, {m.eb}; outputs kept {ok.mean():.2f}"
          + (f"; |C| {np.abs(nz).min():.2e} .. {np.abs(nz).max():.2e}" if nz.size else "; C = 0"))
    if kind == "fewbit":
        assert min(np.mean((P.vl != 0)[P.vh != 0]), np.mean((P.ol != 0)[P.oh != 0])) > 0.6, "both lo planes populated"
        assert (case.A == 0).any() or case.A.size < 40
    if kind == "hionly":
        assert not P.vl.any() and not P.ol.any()
    if kind == "sublo" and shape.K > 1:
        lo = np.concatenate([np.abs(P.vl[P.vl != 0]), np.abs(P.ol[P.ol != 0])])
        assert lo.size and lo.max() <= 2.0 ** -14
    for name, (fn, family, applies) in gc.MUTANTS.items():
        if family not in (case.family, kind):
            continue
        if not applies(case):
            continue
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            bad = fn(case)
        changed = ((bad != m.C) & ~(np.isnan(bad) & np.isnan(m.C))) & ok
        share = float(changed.sum()) / max(int(ok.sum()), 1)
        if share < _share.get(name, (2.0, ""))[0]:
            _share[name] = (share, case.name)
        print(f"    '{name}' changes {int(changed.sum())} of {int(ok.sum())} outputs")
        assert changed.any(), f"'{name}' is not caught by {case.name}"


def test_every_mutant_ran_and_the_summary(capsys):
    """prints what the parametrised tests of this file collected (run alone: goes through the cases itself)"""
    if not _share:
        for case in all_cases():
            check_case(case)
    assert len(gc.MUTANTS) == 17 and set(_share) == set(gc.MUTANTS)
    with capsys.disabled():
        print("\n[sf16 gemm cases] headroom, max T / g per family: " + ", ".join(f"{k} 2^{np.log2(max(v, 1.0)):.2f}" for k, v in _head.items()))
        for name, (share, where) in _share.items():
            print(f"[sf16 gemm cases] '{name}': {100 * share:.1f} % of the outputs on its worst shape ({where})")
