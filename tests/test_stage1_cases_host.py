"""The cases of tests/golden/stage1_cases.py, proved on the host (numpy only, no GPU).

  * the method: a numpy float32 evaluation of tables and query vectors, in two summation orders, equals float64 bit
    for bit on every case; the 2^24 conditions hold (asserted by the generator, re-asserted here); the independent
    packer inverts exactly wherever hi + lo can hold the value and to 2^-22 of the row maximum otherwise;
  * coverage: the union of route() over the case list equals the full label set, and every planted relation count
    is in the generated ids;
  * mutants: each one, applied to the numpy emulation of stage 1 (group build included) or to the packed bytes,
    changes at least one output element on every case it applies to.
A case on which a mutant survives is a badly chosen case: the case is changed, not the mutant.
"""
import functools

import numpy as np
import pytest

import stage1_cases as sc
from exact_cases import LIMIT, round_mantissa

CASES = sc.CASES
RUNS = [(c, dt, e) for c in CASES for dt in c.dtypes for e in c.entries]


def _id(x):
    return x.name if isinstance(x, sc.Stage1Case) else str(x)


# ---------------------------------------------------------------------------------------------- lists -----
def test_names_are_unique_and_every_case_is_small():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES:
        assert c.n_rel * c.r * c.r * 4 <= 16 << 20 and c.B * c.r * 4 <= 16 << 20, c.name
        if c.B >= 2000 and c.n_rel > 8:
            assert c.r <= 8, f"{c.name}: a case about ids keeps b c tiny"


def test_coverage_equals_the_label_set():
    reached = set()
    for c, dt, e in RUNS:
        reached |= sc.route(c, dt, e)
    assert reached == sc.LABELS, (sorted(sc.LABELS - reached), sorted(reached - sc.LABELS))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_planted_counts_and_ids(case):
    core, R, S, rel, sub = sc.operands(case)
    counts = np.bincount(rel, minlength=case.n_rel)
    for i, k in case.rel_ids:
        assert counts[i] == k, (i, k, counts[i])
    assert rel.min() >= 0 and rel.max() < case.n_rel and sub.min() >= 0 and sub.max() < case.n_sub
    assert not S[1 % case.n_sub].any() or case.n_sub == 1
    if case.B >= 2:
        assert (1 % case.n_sub) in sub, "the all-zero subject row is used"
    if case.B > case.n_sub:
        assert len(np.unique(sub)) < case.B, "subjects repeat"


# --------------------------------------------------------------------------------------------- method -----
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fp32_in_two_orders_equals_float64(case):
    core, R, S, rel, sub = sc.operands(case)
    T64, v64 = sc.reference(case)
    t_abs = sc.tables_of(np.abs(core).astype(np.float64), np.abs(R).astype(np.float64))
    assert t_abs.max() < LIMIT
    assert sc.contract(t_abs, np.abs(S).astype(np.float64), rel, sub).max() < LIMIT
    for reverse in (False, True):
        T32 = sc.tables_of(core, R, reverse=reverse)
        assert T32.dtype == np.float32 and np.array_equal(T32.astype(np.float64), T64)
        v32 = sc.contract(T32, S, rel, sub, reverse=reverse)
        assert v32.dtype == np.float32 and np.array_equal(v32.astype(np.float64), v64)
    assert np.abs(v64).max() > 0


@pytest.mark.parametrize("case,dtype,entry", RUNS, ids=_id)
def test_emulation_equals_the_reference(case, dtype, entry):
    T64, v64 = sc.reference(case)
    out = _emulate(case, dtype, entry)
    assert np.array_equal(out["v"], v64)
    _, _, _, rel, _ = sc.operands(case)
    for n, vs in out.get("parts", {}).items():
        for p, v in enumerate(vs):
            mine = rel % n == p
            assert np.array_equal(v[mine], v64[mine]) and np.all(v[~mine] == sc.SENTINEL)


def _holds(x):
    """True where fp16 hi + lo holds x (scaled: |x| < 2^15) exactly, by an independent rule: hi keeps 11 significant
    bits, the rest has to be an fp16 number (11 significant bits, a multiple of 2^-24, below 2^16)."""
    hi = round_mantissa(x, 11).astype(np.float64)
    r = x - hi
    return (round_mantissa(r, 11).astype(np.float64) == r) & (np.rint(r * 2.0 ** 24) == r * 2.0 ** 24)


@pytest.mark.parametrize("case", [c for c in CASES if c.packed], ids=_id)
def test_unpack_inverts_pack(case):
    _, v64 = sc.reference(case)
    v = v64.astype(np.float32)
    for dtype in case.dtypes:
        buf, may = sc.pack_ref(v, dtype)
        back = sc.unpack_ref(buf, case.B, case.r, dtype)
        if dtype == "bf16":
            exact = round_mantissa(v, 8).astype(np.float64) == v64
            assert np.array_equal(back[exact], v64[exact])
            assert np.all(np.abs(back - v64) <= 2.0 ** -8 * np.abs(v64))
            continue
        sh = np.array([sc.pack_shift(np.abs(row).max()) for row in v])[:, None]
        exact = _holds(v64 * 2.0 ** sh)
        assert np.array_equal(back[exact], v64[exact])
        # hi: 11 bits of |x| < 2^15 leave |x - hi| <= 8; lo: 11 bits of that leave 2^-9; the row maximum is >= 2^14
        assert np.all(np.abs(back - v64) <= 2.0 ** -22 * np.abs(v64).max(axis=1, keepdims=True))
        assert exact.mean() > 0.5 or case.regime == "wide12"


def test_unpack_inverts_pack_on_real_rows():
    for B, c in sc.PACK_SHAPES:
        v = sc.pack_rows(B, c, 5)
        buf, may = sc.pack_ref(v, "f32")
        assert len(buf) == ((B + 31) // 32) * (128 + 2 * ((c + 15) // 16) * 1024)
        back = sc.unpack_ref(buf, B, c, "f32")
        mx = np.abs(v).max(axis=1).astype(np.float64)
        ok = (mx >= 2.0 ** -85) & (mx < 2.0 ** 115)                   # rows the +-100 clamp leaves in fp16's range
        assert ok.sum() >= min(B, 3) or B < 3
        assert np.all(np.abs(back - v)[ok] <= 2.0 ** -22 * mx[ok, None])
        assert not may.reshape(-1, len(buf) // ((B + 31) // 32))[-1].all() or B % 32 == 0


def test_some_case_has_bf16_ties_in_both_directions():
    found = []
    for case in CASES:
        if "bf16" not in case.dtypes or not case.packed:
            continue
        _, v64 = sc.reference(case)
        u = v64.astype(np.float32).view(np.uint32)
        tie = (u & 0xFFFF) == 0x8000
        down, up = tie & ((u >> 16) & 1 == 0), tie & ((u >> 16) & 1 == 1)
        if down.any() and up.any():
            found.append(case.name)
            got = sc.bf16_rne(v64.astype(np.float32))
            assert np.array_equal(got[down], (u[down] >> 16).astype(np.uint16))
            assert np.array_equal(got[up], ((u[up] >> 16) + 1).astype(np.uint16))
    assert found, "no case rounds a bf16 tie down and another up"


# -------------------------------------------------------------------------------------------- mutants -----
@functools.lru_cache(maxsize=None)
def _emulate(case, dtype, entry):
    return sc.emulate(case, dtype, entry)


def _outputs_differ(x, y):
    if not np.array_equal(x["v"], y["v"]):
        return True
    return any(not np.array_equal(p, q) for n in x.get("parts", {}) for p, q in zip(x["parts"][n], y["parts"][n]))


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_stage1_mutants_are_seen_on_every_case_they_apply_to(mutant):
    applied = []
    for case, dtype, entry in RUNS:
        if not sc.mutant_applies(mutant, case, dtype, entry):
            continue
        good, bad = _emulate(case, dtype, entry), sc.emulate(case, dtype, entry, mutant)
        assert _outputs_differ(good, bad), f"{mutant} survives on {case.name} ({dtype}, {entry})"
        applied.append(case.name)
    assert len(set(applied)) >= 2, f"{mutant} applies to {sorted(set(applied))} only"


def _pack_mutants(buf, may, v, dtype):
    """{name: bytes} -- the packed bytes a wrong producer would leave (on top of the PACK_FILL pre-fill)."""
    B, c = v.shape
    ks, planes, tile_bytes, ntiles = sc.pack_layout(B, c, dtype)
    good = np.where(may, buf, np.uint8(sc.PACK_FILL))
    out = {}
    tiles = lambda x: x.reshape(ntiles, tile_bytes)                      # noqa: E731
    if dtype == "f32":
        m = good.copy()
        lo = tiles(m)[:, sc.PACK_HDR + ks * 1024:]
        lo[tiles(may)[:, sc.PACK_HDR + ks * 1024:]] = 0
        out["lo_plane_zero"] = m
        m = good.copy()
        hdr = tiles(m)[:, :sc.PACK_HDR].copy().view(np.float32)
        hdr[tiles(may)[:, :sc.PACK_HDR].copy().view(np.uint32) != 0] *= 2
        tiles(m)[:, :sc.PACK_HDR] = hdr.view(np.uint8)
        out["header_times_two"] = m
    m = good.copy()
    pl = tiles(m)[:, sc.PACK_HDR:].copy().view(np.uint16).reshape(ntiles, planes, ks, 2, 32, 8)
    tiles(m)[:, sc.PACK_HDR:] = pl[:, :, :, ::-1].copy().reshape(ntiles, -1).view(np.uint8)
    out["k_half_swapped"] = m
    if c % 16:
        m = good.copy()
        tiles(m)[0, sc.PACK_HDR:].view(np.uint16)[sc.pack_offset(ks * 16 - 1, 0)] = 0x3C00
        out["k_padding_not_zero"] = m
    if B % 32:
        m = good.copy()
        tiles(m)[-1, sc.PACK_HDR:].view(np.uint16)[sc.pack_offset(0, B % 32)] = 0
        out["row_past_B_written"] = m
    if dtype == "bf16":
        m = good.copy()
        k = np.arange(c)
        for d in range(B):
            tiles(m)[d >> 5, sc.PACK_HDR:].view(np.uint16)[sc.pack_offset(k, d & 31)] = (v[d].view(np.uint32) >> 16).astype(np.uint16)
        out["bf16_truncated"] = m
    return good, out


@pytest.mark.parametrize("case", [c for c in CASES if c.packed and c.B <= 64], ids=_id)
def test_packer_mutants_are_seen(case):
    _, v64 = sc.reference(case)
    v = v64.astype(np.float32)
    for dtype in case.dtypes:
        buf, may = sc.pack_ref(v, dtype)
        good, mutants = _pack_mutants(buf, may, v, dtype)
        assert sc.packed_mismatch(good, v, dtype) is None
        for name, m in mutants.items():
            if np.array_equal(m, good):
                continue                                   # a no-op here (all lo halves zero, all values bf16 numbers)
            assert sc.packed_mismatch(m, v, dtype) is not None, f"{name} survives on {case.name} ({dtype})"


def test_every_packer_mutant_was_seen_somewhere():
    seen = set()
    for case in [c for c in CASES if c.packed and c.B <= 64]:
        _, v64 = sc.reference(case)
        v = v64.astype(np.float32)
        for dtype in case.dtypes:
            buf, may = sc.pack_ref(v, dtype)
            good, mutants = _pack_mutants(buf, may, v, dtype)
            seen |= {name for name, m in mutants.items() if sc.packed_mismatch(m, v, dtype) is not None}
    assert seen == {"lo_plane_zero", "header_times_two", "k_half_swapped", "k_padding_not_zero", "row_past_B_written",
                    "bf16_truncated"}
