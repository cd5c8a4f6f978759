"""Host proof of the tall-Gram cases (tests/golden/tall_gram_cases.py): the cases reach every branch the kernel and
its launcher have, the split rule keeps its promises, a float64 emulation of the kernel's split in another summation
order meets every case's bound (so the bound does not depend on the order), and each defect the kernel could have
leaves the bound -- or bit equality -- on at least one case (so the GPU test that applies the same bounds to the
kernel would see it).  No GPU, no library."""
import numpy as np
import pytest

import tall_gram_cases as tg


def test_cases_reach_every_label():
    reached = set()
    for c in tg.CASES:
        f = tg.features(c)
        assert f <= tg.LABELS, f - tg.LABELS
        reached |= f
    assert reached == tg.LABELS, tg.LABELS - reached
    assert len({c.name for c in tg.CASES}) == len(tg.CASES)
    # the issue's grid: every n with every shape (contiguous), both families; both load paths in both families
    for fam in tg.FAMILIES:
        names = {(c.n, c.p, c.q) for c in tg.CASES if c.family == fam and c.layout == "contig"}
        assert names == {(n, p, q) for n in tg.NS for p, q in tg.SHAPES}
        assert {tg.vector_path(c) for c in tg.CASES if c.family == fam} == {True, False}
        assert {c.layout for c in tg.CASES if c.family == fam} == set(tg.LAYOUTS)


def test_split_rule():
    """Static in (n, p, q); ranges of equal length, a multiple of the chunk, that cover [0, n) with a non-empty last
    one; the workspace is the partials, 256-byte aligned, at most 64 MiB and bounded in n."""
    for p, q in tg.SHAPES + ((1024, 1024), (1000, 7), (65, 1024)):
        for n in tg.NS + (0, 1024, 1025, 40943, 125000, 65536, 10 ** 7, 2 ** 33):
            length, ranges = tg.split(n, p, q)
            assert length % tg.KC == 0 and length >= tg.MIN_ROWS and ranges >= 1
            assert (ranges - 1) * length < max(n, 1) <= ranges * length or n == 0
            ws = tg.workspace_bytes(n, p, q)
            assert ws % 256 == 0 and ranges * p * q * 8 <= ws <= tg.WS_MAX
            assert ranges * tg.tiles(p, q) <= tg.TARGET_WG or ranges == 1
    assert tg.split(2500, 8, 8) == (1024, 3) and tg.split(4099, 512, 512) == (1024, 5)
    assert tg.split(125000, 512, 512) == (7840, 16) and tg.split(40943, 200, 200) == (1024, 40)
    assert tg.workspace_bytes(10, 0, 4) == 0 and tg.workspace_bytes(10, 4, 1025) == 0 and tg.workspace_bytes(-1, 4, 4) == 0
    assert tg.workspace_bytes(0, 4, 4) == 256
    assert tg.workspace_bytes(10 ** 9, 1024, 1024) == 4 * 1024 * 1024 * 8          # four ranges: 256 tiles each


@pytest.fixture(scope="module")
def verdicts():
    """For every case: the emulation's and every mutant's ``(ok, worst)``; reference and bound are formed once."""
    out = {}
    for c in tg.CASES:
        ref, bnd = tg.reference(c), tg.bound(c)
        out[c.name] = {m: tg.inside(c, tg.emulate(c, m), ref, bnd) for m in (None,) + tg.MUTANTS}
    return out


def test_another_summation_order_stays_inside(verdicts):
    worst = 0.0
    for c in tg.CASES:
        ok, w = verdicts[c.name][None]
        assert ok, (c.name, w)
        worst = max(worst, w) if c.family == "G" else worst
    print(f"float64 emulation in another order: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("mutant", tg.MUTANTS)
def test_mutant_leaves_the_bound(verdicts, mutant):
    caught = [c.name for c in tg.CASES if not verdicts[c.name][mutant][0]]
    print(f"{mutant}: caught on {len(caught)} of {len(tg.CASES)} cases, e.g. {caught[:3]}")
    assert caught
    for fam in tg.FAMILIES:        # each family's check alone sees it
        assert any(tg.BY_NAME[nm].family == fam for nm in caught), (mutant, fam)


def test_family_e_is_exact_and_family_g_is_full_mantissa():
    for c in tg.CASES:
        A, B = tg.matrices(c)
        if c.family == "E":
            assert np.abs(A).max() <= 1024 and (A == np.round(A)).all() and (B == np.round(B)).all()
            assert c.n * 2.0 ** 20 < 2.0 ** 53
        elif c.n * c.p >= 1000:
            assert (A.view(np.uint32) & 1).mean() > 0.3        # the last mantissa bit is in use
