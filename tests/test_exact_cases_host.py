"""The exact-operand method of tests/golden/exact_cases.py, proved on the host (numpy only, no GPU).

For every case the GPU files run (the same lists, at full size):
  * the generator's 2^24 condition holds (asserted inside the generator);
  * a numpy float32 evaluation of the same formulas equals the float64 reference bit for bit, in two summation
    orders: the natural one, and reversed / chunked like a split-K;
  * every mutant that applies to the case changes at least one element: one term dropped, one term counted twice,
    the K tail read one element too far / too short, the wide operand rounded to 11 and to 8 mantissa bits (wide
    regimes), ids compared after truncation to 13 bits (cases that hold two ids equal modulo 8192).
A case on which a mutant survives is a badly chosen case: the case is changed, not the mutant.
"""
import numpy as np
import pytest

import exact_cases as ec

GEMM_EXACT = [c for c in ec.GEMM_CASES if c.exact]
BWD_EXACT = [c for c in ec.BWD_CASES + [ec.BWD_NULL_CASE] if c.exact]


def _same(x, ref):
    return np.array_equal(np.asarray(x, dtype=np.float64), ref)


# ---------------------------------------------------------------------------------------------- lists -----
def test_case_names_are_unique_and_lists_cover_the_issue():
    names = [c.name for c in ec.GEMM_CASES + ec.GEMM_SIGMOID_CASES] + [c.name for c in ec.BWD_CASES]
    assert len(names) == len(set(names))
    g = [c for c in ec.GEMM_CASES if c.splits == 0 and c.entry == "gemm"]
    assert {c.M for c in g} >= {1, 31, 127, 128, 129, 257} and {c.N for c in g} >= {1, 31, 127, 128, 129, 257}
    assert {c.K for c in g} >= {1, 2, 7, 8, 9, 15, 16, 17, 33, 157, 1000}
    assert {(c.ak, c.bk) for c in g} == {(1, 1), (1, 0), (0, 1), (0, 0)}
    assert {c.splits for c in ec.GEMM_CASES if c.splits} >= {1, 2, 7, 16}
    assert max(c.K for c in ec.GEMM_CASES if c.regime.startswith("wide")) == 40943
    widths = {c.a for c in ec.BWD_CASES} | {c.b for c in ec.BWD_CASES}
    assert widths >= {1, 2, 7, 100, 128, 129, 256, 257, 512, 513, 768, 769, 1024}
    assert {c.B for c in ec.BWD_CASES} >= {1, 255, 256, 257, 8192, 8193, 20000}
    assert {ec.gcore_splits(c.B, c.a, c.b, c.c) for c in ec.BWD_CASES} >= {1, 4, 16}
    assert {c.wide for c in ec.BWD_CASES if c.regime.startswith("wide")} == {"dv", "core"}


def test_window_counts_of_the_scatter_cases():
    """scatter_rows_kernel compacts the matches of an id per 256-query window (windows start at the id's first query)
    and unrolls over that window's count: 8 rows on the register path, 8 * slots on the slots path (slots = 256 // w).
    The edge counts must occur as per-window counts, in a first window and in a later one -- not as total lengths."""
    by = {c.name: c for c in ec.BWD_CASES}

    def counts(name, which):
        ops = ec.bwd_operands(by[name])
        wc = ec.window_counts(ops[4 if which == "rel" else 5])
        return {w[0] for w in wc.values()}, {x for w in wc.values() for x in w[1:]}, {sum(w) for w in wc.values()}
    first, later, total = counts("regs_lists", "sub")                         # b = 200: register path
    assert first >= {1, 7, 8, 9, 255, 256} and later >= {7, 8, 9, 1} and total >= {1, 7, 8, 9, 255, 256, 257}
    assert ec.window_counts(ec.bwd_operands(by["regs_list_all"])[5]) == {9: [256, 256, 188]}       # length B
    for which in ("sub", "rel"):                                               # w = 40: slots = 6, edge 48
        first, later, _ = counts("slots_lists_w40", which)
        assert 256 // 40 == 6 and first >= {47, 48, 49, 97} and later >= {47, 48, 49}
    first, later, _ = counts("slots_lists_w128_w64", "sub")                    # w = 128: slots = 2, edge 16
    assert by["slots_lists_w128_w64"].b == 128 and first >= {15, 16, 17, 33} and later >= {15, 16, 17}
    first, later, _ = counts("slots_lists_w128_w64", "rel")                    # w = 64: slots = 4, edge 32
    assert by["slots_lists_w128_w64"].a == 64 and first >= {31, 32, 33, 65} and later >= {31, 32, 33}
    ops = ec.bwd_operands(by["batch_20000_late_first"])
    for ids, j in ((ops[5], 39999), (ops[5], 0), (ops[4], 8), (ops[4], 8 + 8192)):
        assert np.flatnonzero(ids == j)[0] >= 8192                           # first occurrence beyond query 8192
    assert ec.window_counts(ops[5])[39999][:5] == [200, 200, 200, 100, 0] and ec.window_counts(ops[4])[8][:4] == [200, 200, 113, 0]
    ops = ec.bwd_operands(by["batch_8193_high_bits"])
    assert {5, 5 + 8192, 5 + 16384} <= set(ops[5].tolist()) and {77, 77 + 8192} <= set(ops[4].tolist())


# ---------------------------------------------------------------------------------------------- GEMM ------
def _gemm_f32(A, B, order, chunks):
    """A . B^T evaluated in float32; "reversed": k runs backwards in `chunks` partial sums added in fp32."""
    A, B = A.astype(np.float32), B.astype(np.float32)
    if order == "natural":
        return A @ B.T
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for idx in np.array_split(np.arange(A.shape[1])[::-1], chunks):
        if len(idx):
            acc = acc + (A[:, idx] @ B[:, idx].T).astype(np.float32)
    return acc


@pytest.mark.parametrize("case", GEMM_EXACT, ids=lambda c: c.name)
def test_gemm_case_is_exact_in_fp32_and_catches_every_mutant(case):
    A1, B1 = ec.gemm_operands(case, extra_k=1)            # the generator asserts the 2^24 condition
    A, B = A1[:, :case.K], B1[:, :case.K]
    ref = ec.gemm_ref(A, B)
    assert np.abs(ref).max() < ec.LIMIT and np.array_equal(ref, np.rint(ref))
    assert _same(_gemm_f32(A, B, "natural", 1), ref)
    assert _same(_gemm_f32(A, B, "reversed", max(case.splits, 3)), ref)
    # mutants -----------------------------------------------------------------------------------------------
    k = int(np.flatnonzero(np.abs(A).max(axis=0) * np.abs(B).max(axis=0) > 0)[0])
    m, n = int(np.flatnonzero(A[:, k])[0]), int(np.flatnonzero(B[:, k])[0])
    assert A[m, k] != 0 and B[n, k] != 0                  # the term (m, n, k) is non-zero: that is what the case must offer
    Ad = A.copy()
    Ad[m, k] = 0                                           # dropped: the product recomputed without a(m, k)
    assert not np.array_equal(ec.gemm_ref(Ad, B), ref), "one term dropped"
    A2 = np.concatenate([A, np.zeros((case.M, 1), np.float32)], axis=1)
    B2 = np.concatenate([B, np.zeros((case.N, 1), np.float32)], axis=1)
    A2[m, -1], B2[n, -1] = A[m, k], B[n, k]                # doubled: the term (m, n, k) a second time
    assert not np.array_equal(ec.gemm_ref(A2, B2), ref), "one term counted twice"
    assert not np.array_equal(ec.gemm_ref(A1, B1), ref), "K tail read one element too far"
    if case.K > 1:
        assert not np.array_equal(ec.gemm_ref(A[:, :-1], B[:, :-1]), ref), "K tail read one element too short"
    else:
        assert np.all(ref != 0)                            # K = 1: a kernel that stops short returns zeros
    if case.regime.startswith("wide"):
        for bits in (11, 8):
            Am, Bm = (ec.round_mantissa(A, bits), B) if case.wide == "A" else (A, ec.round_mantissa(B, bits))
            assert not np.array_equal(ec.gemm_ref(Am, Bm), ref), f"wide operand rounded to {bits} bits"


@pytest.mark.parametrize("case", [c for c in ec.GEMM_CASES + ec.GEMM_SIGMOID_CASES if not c.exact], ids=lambda c: c.name)
def test_gemm_real_case_fp32_chain_is_inside_the_gamma_bound(case):
    """The bound of the real-valued layer is derived, not measured; a float32 chain on the host stays inside it."""
    assert case.K <= 256
    A, B = ec.gemm_operands(case)
    ref, bound = ec.gemm_ref(A, B), ec.gemm_bound(case, A, B)
    acc = np.zeros((case.M, case.N), dtype=np.float32)
    for k in range(case.K):                                 # a k-ordered chain (products rounded: no looser than fma)
        acc = acc + A[:, k:k + 1] * B[:, k:k + 1].T
    assert np.all(np.abs(acc.astype(np.float64) - ref) <= 2 * bound)   # two roundings per step here, one in an fma


# -------------------------------------------------------------------------------- stage-1 backward ------
def _first_nonzero_row(rows, members):
    for d in members:
        if np.any(rows[d] != 0):
            return int(d)
    raise AssertionError("no query of the longest list has a non-zero row: badly chosen case")


@pytest.mark.parametrize("case", BWD_EXACT, ids=lambda c: c.name)
def test_bwd_case_is_exact_in_fp32_and_catches_every_mutant(case):
    core, R, S, dv, rel, sub = ec.bwd_operands(case)      # asserts the 2^24 condition on g_core, g_R and g_S
    ref = ec.bwd_ref(core, R, S, dv, rel, sub)
    for g in ref:
        assert np.abs(g).max() < ec.LIMIT and np.array_equal(g, np.rint(g))
    splits = ec.gcore_splits(case.B, case.a, case.b, case.c)
    for order, chunks in (("natural", 1), ("reversed", max(splits, 3))):
        got = ec.bwd_ref(core, R, S, dv, rel, sub, dtype=np.float32, order=order, chunks=chunks)
        for g, e in zip(got, ref):
            assert g.dtype == np.float32 and _same(g, e), order
    # ids absent from the batch have zero rows, the others are (mostly) not: the test can see a misplaced row
    for g, ids in ((ref[1], rel), (ref[2], sub)):
        absent = np.setdiff1d(np.arange(g.shape[0]), ids)
        assert not g[absent].any()
    rows_R, rows_S = ec.bwd_rows(core, R, S, dv, rel, sub)
    assert np.mean(np.any(rows_R != 0, axis=1)) >= 0.5 and np.mean(np.any(rows_S != 0, axis=1)) >= 0.5
    # mutants: one query dropped from / counted twice in the longest list of each table -- the gradients recomputed
    # on the batch without that query / with it a second time.  (What makes them visible is that the query's row is
    # non-zero, which _first_nonzero_row demands of the case.)
    for gi, ids, rows in ((1, rel, rows_R), (2, sub, rows_S)):
        j = int(np.argmax(np.bincount(ids)))
        d = _first_nonzero_row(rows, np.flatnonzero(ids == j)[::-1])
        keep = np.delete(np.arange(case.B), d)
        twice = np.append(np.arange(case.B), d)
        for sel in (keep, twice):
            if len(sel):
                mut = ec.bwd_ref(core, R, S, dv[sel], rel[sel], sub[sel])
                assert not np.array_equal(mut[gi], ref[gi])
    Xdv = np.einsum("da,db,dc->dabc", R[rel].astype(np.float64), S[sub].astype(np.float64), dv.astype(np.float64)) \
        if case.B * case.a * case.b * case.c <= 2 ** 24 else None
    if Xdv is not None:
        assert np.mean(Xdv.reshape(case.B, -1).any(axis=1)) >= 0.5     # most queries are visible in g_core
    # the c chain read one element too far / too short
    junk = np.random.default_rng(1)                       # (varied: a constant can cancel against a zero-sum row of R)
    far = ec.bwd_ref(np.concatenate([core, junk.integers(3, 8, (case.a, case.b, 1)).astype(np.float32)], axis=2), R, S,
                     np.concatenate([dv, junk.integers(3, 8, (case.B, 1)).astype(np.float32)], axis=1), rel, sub)
    assert not np.array_equal(far[1], ref[1]) and not np.array_equal(far[2], ref[2])
    if case.c > 1:
        short = ec.bwd_ref(core[:, :, :-1], R, S, dv[:, :-1], rel, sub)
        assert not np.array_equal(short[1], ref[1]) and not np.array_equal(short[2], ref[2])
    # the batch chain of g_core one query too short
    if case.B > 1:
        last = np.einsum("a,b,c->abc", R[rel[-1]].astype(np.float64), S[sub[-1]].astype(np.float64), dv[-1].astype(np.float64))
        if last.any():
            assert not np.array_equal(ref[0] - last, ref[0])
    if case.regime.startswith("wide"):
        for bits in (11, 8):
            ops = {"core": core, "dv": dv}
            ops[case.wide] = ec.round_mantissa(ops[case.wide], bits)
            mut = ec.bwd_ref(ops["core"], R, S, ops["dv"], rel, sub)
            assert all(not np.array_equal(m, e) for m, e in zip(mut[1:], ref[1:])), f"{case.wide} rounded to {bits} bits"
            if case.wide == "dv":
                assert not np.array_equal(mut[0], ref[0])
    # ids compared after truncation to 13 bits: applies where two ids of the batch agree modulo 8192
    # (a kernel that does so adds the queries of all ids with one truncated value to the row of the first of them)
    for gi, ids in ((1, rel), (2, sub)):
        u = np.unique(ids)
        if len(np.unique(u & 8191)) < len(u):
            first = {}
            for i in ids:
                first.setdefault(int(i) & 8191, int(i))
            merged = np.array([first[int(i) & 8191] for i in ids])
            mut = ec.bwd_ref(core, R, S, dv, merged if gi == 1 else rel, merged if gi == 2 else sub)
            assert not np.array_equal(mut[gi], ref[gi])


def test_truncated_id_mutant_applies_somewhere():
    hit = {"rel": 0, "sub": 0}
    for case in BWD_EXACT:
        if max(case.n_rel, case.n_sub) > 8192:
            _, _, _, _, rel, sub = ec.bwd_operands(case)
            for k, ids in (("rel", rel), ("sub", sub)):
                u = np.unique(ids)
                hit[k] += len(np.unique(u & 8191)) < len(u)
    assert hit["rel"] >= 1 and hit["sub"] >= 1


@pytest.mark.parametrize("case", [c for c in ec.BWD_CASES if not c.exact], ids=lambda c: c.name)
def test_bwd_real_case_shape_limits_and_fp32_inside_bound(case):
    core, R, S, dv, rel, sub = ec.bwd_operands(case)
    assert case.c <= 64 and np.bincount(rel).max() <= 200 and np.bincount(sub).max() <= 200
    splits = ec.gcore_splits(case.B, case.a, case.b, case.c)
    ref = ec.bwd_ref(core, R, S, dv, rel, sub)
    bounds = ec.bwd_bounds(case, core, R, S, dv, rel, sub, splits)
    got = ec.bwd_ref(core, R, S, dv, rel, sub, dtype=np.float32)
    for g, e, bd in zip(got, ref, bounds):
        assert np.all(np.abs(g.astype(np.float64) - e) <= bd)
