"""The cases of tests/golden/scatter_cases.py, proved on the host (numpy only, no GPU).

  * the method: every product dz v is a float32 number, so the emulation's float32 adds are the kernels' fmaf; the
    emulation agrees with float64 within gamma(n - 1) sum |dz v| per element (n = the run's length);
  * coverage: the union of features() over the case list equals the label set; the planted runs lie where the case
    list says they do;
  * mutants: a window twice as long, descending order within an entity, the combine order reversed and a chain
    carried across window boundaries each change the bits of at least one case.
A mutant that changes nothing means the cases are too tame: the cases are changed, not the mutant.
"""
import numpy as np
import pytest

import scatter_cases as sc

CASES = sc.CASES
by_name = dict(ids=lambda c: c.name)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_names_are_unique_and_every_case_is_small():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    for c in CASES:
        assert c.c <= sc.MAXC and c.n_ent * c.c * 4 <= 2 << 20 and c.M <= 70_000, c.name
        assert c.M <= 4096 or c.c == 4, f"{c.name}: a case about M keeps c tiny"


def test_coverage_equals_the_label_set():
    reached = set()
    for c in CASES:
        reached |= sc.features(c)
    assert reached == sc.LABELS, (sorted(sc.LABELS - reached), sorted(reached - sc.LABELS))


def test_window_rule_and_radix_passes():
    assert [sc.cand_window(m) for m in (1, 65536, 65537, 131072, 131073, 10 ** 6, 2 ** 30)] == [16, 16, 32, 32, 48, 256, 256]
    assert [sc.radix_passes(n) for n in (255, 256, 65535, 65536)] == [1, 2, 2, 3]
    assert sc.BY_NAME["win32"].win == 32 and all(c.win == 16 for c in CASES if c.name != "win32")


def test_planted_runs_lie_where_the_list_says():
    case = sc.BY_NAME["planted_c6"]
    cand, _, _ = sc.operands(case)
    _, runs = sc.sorted_runs(case, cand)
    assert [(s, t) for _, s, t in runs] == [(0, 5), (5, 16), (16, 32), (32, 35), (35, 55), (55, 105), (105, 112),
                                            (112, 152), (152, 154)]
    assert sc.features(case) >= {"inside", "two_windows", "three_plus", "ends_on_window_end", "starts_on_window_start",
                                 "both_slots", "last_window_partial", "negative_id", "large_id", "run_before_invalid",
                                 "unroll8_tail", "no_vector"}
    shared = sc.BY_NAME["shared_list"]
    cand, _, _ = sc.operands(shared)
    assert cand.shape[0] == 1
    assert all(t - s == shared.B for _, s, t in sc.sorted_runs(shared, cand)[1])


@pytest.mark.parametrize("case", CASES, **by_name)
def test_operands_are_12_bit_and_products_exact(case):
    cand, dz, v = sc.operands(case)
    K = case.K
    for x in (dz[:, :K], v):
        assert x.dtype == np.float32 and np.array_equal(sc.round_mantissa(x, 12), x)
    if case.dz_pad:
        assert np.all(dz[:, K:] == sc.SENTINEL)
    if case.M:
        d = np.arange(case.B)
        p32 = dz[d, 0][:, None] * v
        assert p32.dtype == np.float32
        assert np.array_equal(p32.astype(np.float64), dz[d, 0].astype(np.float64)[:, None] * v.astype(np.float64))
    keys = sc.keys_of(case, cand)
    assert keys.size == case.M and (keys >= 0).all() and (keys <= case.n_ent).all()


@pytest.mark.parametrize("case", CASES, **by_name)
def test_emulation_within_the_float64_bound(case):
    g64, bound = sc.reference(case)
    got = sc.expected(case)
    assert got.dtype == np.float32 and got.shape == (case.n_ent, case.c)
    err = np.abs(got.astype(np.float64) - g64)
    assert (err <= bound).all(), f"max excess {(err - bound).max():.3e}"
    named = np.zeros(case.n_ent, dtype=bool)
    keys = sc.keys_of(case, sc.operands(case)[0])
    named[keys[keys < case.n_ent]] = True
    assert not bits(got[~named]).any(), "a row without entries is not +0"
    if case.M:
        assert (err > 0).any() or case.M == 1, "nothing rounds: the exponents are too tame"


@pytest.mark.parametrize("mutant", sorted(sc.MUTANTS))
def test_each_mutant_changes_the_bits_of_some_case(mutant):
    changed = [c.name for c in CASES if c.M and c.M <= 4096
               and not np.array_equal(bits(sc.MUTANTS[mutant](c)), bits(sc.expected(c)))]
    print(f"\n[{mutant}] changes {len(changed)} cases: {', '.join(changed)}")
    assert changed, f"no case sees the mutant '{mutant}'"
    assert "planted_c6" in changed, "the planted runs are meant to see every mutant"


def test_the_win32_case_tells_16_from_32():
    case = sc.BY_NAME["win32"]
    assert not np.array_equal(bits(sc.emulate(case, win=16)), bits(sc.expected(case)))
