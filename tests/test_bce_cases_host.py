"""The method of tests/golden/bce_cases.py, proved on the host (numpy only, no GPU).

For every case the GPU file runs (the same lists, at full size) numpy float32 emulations of the four kernels
(bce_rows_kernel, bce_grad_pos_kernel + bce_grad_all_kernel, bce_patch_pos_kernel and the loss epilogue of
score_split_kernel), each in two lane orders, stay inside the bounds / equal the bit patterns, and every mutant that
applies to a case fails it:
  stride    a positive at list index >= the loop stride (256 / 64 / 16) is dropped
  tail      the last partial unroll block (rows: N % 2048; gradient: N % 4 on the vector path) is skipped
  wrap      an out-of-range id is taken modulo N instead of skipped
  dup       a slot that two batch rows share is served for the first of them only
  unsat     a saturated entry is not zeroed (gradient)
  sign      the sign of the stored zero is swapped (fused epilogue, patch kernel)
  flush     L reads a subnormal as 0, i.e. -100 (the row kernel before this file existed)
  dt_zero   a positive whose score equals dt comes back as 0 (the gradient kernels before this file existed)
  marker    x == t0 is stored as 0 and not as the smallest denormal (fused epilogue)
A case on which an applicable mutant survives is a badly chosen case: the case is changed, not the mutant.
"""
import numpy as np
import pytest

import bce_cases as bc

F32 = np.float32
LN2 = F32(0.6931471805599453)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def clog32(x, flush=False):
    """fp32 ln on a correctly rounded log2, scaled and clamped as the kernels do it."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    if flush:
        x64 = np.where(x64 < 2.0 ** -126, 0.0, x64)
    with np.errstate(divide="ignore"):
        l2 = np.log2(x64).astype(np.float32)
    return np.maximum(l2 * LN2, F32(-100))


def _lists(case, csr, d, mut, stride, seen):
    """List entries of row d as the (possibly mutated) kernel walks them: ids, with -1 for a skipped entry."""
    l = csr.list_of(d).copy()
    if mut == "dup" and csr.slot[d] in seen:
        return l[:0]
    if mut == "stride":
        l = l[:stride]
    if mut == "wrap":
        return l % case.N
    return np.where((l >= 0) & (l < case.N), l, -1)


# ---------------------------------------------------------------------------------------------- rows ------
def emu_rows(case, csr, P, lanes=256, reverse=False, mut=None):
    N = case.N
    t0, dt = bc.constants(N, case.eps)
    out, seen = np.zeros(case.B), set()
    n_main = (N // 2048) * 2048 if mut == "tail" else N
    for d in range(case.B):
        p = P[d, :n_main]
        term = t0 * clog32(p, mut == "flush") + (bc.F1 - t0) * clog32(bc.F1 - p, mut == "flush")
        acc = np.zeros(lanes, dtype=np.float32)
        starts = list(range(0, n_main, lanes))
        for a in (reversed(starts) if reverse else starts):
            ch = term[a:a + lanes]
            acc[:len(ch)] += ch
        l = _lists(case, csr, d, mut, 256, seen)
        seen.add(csr.slot[d])
        for a in range(0, len(l), lanes):
            ids = l[a:a + lanes]
            ok = ids >= 0
            q = P[d, ids[ok]]
            acc[:len(ids)][ok] += dt * (clog32(q, mut == "flush") - clog32(bc.F1 - q, mut == "flush"))
        out[d] = -acc.astype(np.float64).sum()
    return out


def rows_setup(case):
    csr = bc.build_csr(np.random.default_rng(bc._seed(case.name)), case.N, case.lengths, case.B)
    P, pos = bc.plant(case, csr)
    ref, mag = bc.rows_reference(case, P, pos)
    return csr, P, pos, ref, bc.rows_bound(case.N, max(case.lengths), mag, ref), mag


def rows_mutants(case, csr, P, pos):
    N = case.N
    m = []
    if any(((csr.list_of(d)[256:] >= 0) & (csr.list_of(d)[256:] < N)).any() for d in range(case.B)):
        m.append("stride")
    if N % 2048:
        m.append("tail")
    wrapped = [(d, j % N) for d in range(case.B) for j in csr.list_of(d) if not 0 <= j < N]
    if any(not pos[d, j] for d, j in wrapped):
        m.append("wrap")
    first = {}
    if any(first.setdefault(csr.slot[d], d) != d and len(csr.positives(d, N)) for d in range(case.B)):
        m.append("dup")
    sub = (P[:, :N] < F32(2.0 ** -126)) & (P[:, :N] > F32(1e-43)) & pos          # ln p > -100: the clamp does not hide it
    if sub.any():
        m.append("flush")
    return m


@pytest.mark.parametrize("case", bc.ROWS_CASES + bc.BOUND_TRIALS, ids=lambda c: c.name)
def test_rows_emulations_pass_and_mutants_fail(case):
    csr, P, pos, ref, bound, mag = rows_setup(case)
    for lanes, rev in ((256, False), (64, True)):
        err = np.abs(emu_rows(case, csr, P, lanes, rev) - ref)
        assert np.all(err <= bound), (lanes, float((err / bound).max()))
    if case in bc.BOUND_TRIALS:
        # against the issue's own bound (not the capped one): correctly rounded logs use a small part of it
        k = -(-case.N // 256) + -(-max(case.lengths) // 256) + 16
        own = k * bc.U * mag + case.N * 2.0 ** -23
        assert float((np.abs(emu_rows(case, csr, P) - ref) / own).max()) <= 0.03
    for mut in rows_mutants(case, csr, P, pos):
        err = np.abs(emu_rows(case, csr, P, mut=mut) - ref)
        assert np.any(err > bound), f"mutant {mut} survives {case.name}"


# ---------------------------------------------------------------------------------------------- grad ------
def emu_grad(case, csr, P, reverse=False, mut=None, vec=True):
    N = case.N
    t0, dt = bc.constants(N, case.eps)
    s = bc.grad_factor(bc.GRAD_G, 1.0 / (case.B * N))
    X, seen = P[:, :N].copy(), set()
    for d in range(case.B):
        l = _lists(case, csr, d, mut, 64, seen)
        seen.add(csr.slot[d])
        for j in (l[::-1] if reverse else l):
            if j < 0:
                continue
            p = X[d, j]
            if p != 1.0 and p != 0.0:
                X[d, j] = p - dt if (mut == "dt_zero" or p != dt) else bc.DENORM_MIN
    sat = (X == 1.0) | (X == 0.0)
    out = ((X - t0) * s).astype(np.float32)
    if mut != "unsat":
        out = np.where(sat, F32(0), out)
    if mut == "tail" and vec:
        out[:, N - N % 4:] = X[:, N - N % 4:]
    return out


def grad_setup(case):
    csr = bc.build_csr(np.random.default_rng(bc._seed(case.name)), case.N, case.lengths, case.B)
    P, pos = bc.plant(case, csr)
    return csr, P, pos, bc.grad_reference(case, P, pos)


def grad_is_vec(case):
    return case.ld % 4 == 0 and case.off % 4 == 0


def grad_mutants(case, csr, P, pos):
    N = case.N
    t0, dt = bc.constants(N, case.eps)
    m = ["unsat"]
    if any(((csr.list_of(d)[64:] >= 0) & (csr.list_of(d)[64:] < N)).any() for d in range(case.B)):
        m.append("stride")
    if grad_is_vec(case) and N % 4:
        m.append("tail")
    if any(not pos[d, j % N] for d in range(case.B) for j in csr.list_of(d) if not 0 <= j < N):
        m.append("wrap")
    first = {}
    if any(first.setdefault(csr.slot[d], d) != d and len(csr.positives(d, N)) for d in range(case.B)):
        m.append("dup")
    if dt != 1.0 and ((P[:, :N] == dt) & pos).any():
        m.append("dt_zero")
    return m


@pytest.mark.parametrize("case", bc.GRAD_CASES, ids=lambda c: c.name)
def test_grad_emulations_equal_and_mutants_differ(case):
    csr, P, pos, ref = grad_setup(case)
    for rev in (False, True):
        assert np.array_equal(bits(emu_grad(case, csr, P, rev)), bits(ref))
    for mut in grad_mutants(case, csr, P, pos):
        assert not np.array_equal(bits(emu_grad(case, csr, P, mut=mut, vec=grad_is_vec(case))), bits(ref)), \
            f"mutant {mut} survives {case.name}"


def test_a_positive_at_dt_has_the_contract_gradient():
    case = next(c for c in bc.GRAD_CASES if c.name == "vec_n259")
    csr, P, pos, ref = grad_setup(case)
    t0, dt = bc.constants(case.N, case.eps)
    hit = (P[:, :case.N] == dt) & pos
    assert hit.any()
    s = bc.grad_factor(bc.GRAD_G, 1.0 / (case.B * case.N))
    assert np.all(bits(ref[hit]) == bits(-t0 * s)) and (-t0 * s) != 0


# ---------------------------------------------------------------------------------------------- patch -----
def emu_patch(case, csr, X, z, chains=16, reverse=False, mut=None):
    N = case.N
    t0, dt = bc.constants(N, case.eps)
    out, corr, seen = X.copy(), np.zeros(case.B), set()
    for d in range(case.B):
        l = _lists(case, csr, d, mut, 16, seen)
        seen.add(csr.slot[d])
        acc = np.zeros(chains, dtype=np.float32)
        order = list(enumerate(l))
        for i, j in (reversed(order) if reverse else order):
            if j < 0:
                continue
            x = X[d, j]
            if x == 0.0:
                neg = bool(np.signbit(x)) != (mut == "sign")
                acc[i % chains] += -dt * F32(100) if neg else dt * F32(100)
                continue
            zz = F32(z[d, j])
            assert float(zz) == z[d, j]
            e = F32(np.exp2(np.float64(zz * F32(-1.4426950408889634))))
            p = F32(1.0 / np.float64(F32(1) + e))
            acc[i % chains] += dt * (clog32(p) - clog32(F32(1) - p))
            out[d, j] = x - dt
        corr[d] = -acc.astype(np.float64).sum()
    return out, corr


def patch_mutants(case, csr, X):
    N = case.N
    pos = np.zeros((case.B, N), dtype=bool)
    for d in range(case.B):
        pos[d, csr.positives(d, N)] = True
    m = []
    if any(((csr.list_of(d)[16:] >= 0) & (csr.list_of(d)[16:] < N)).any() for d in range(case.B)):
        m.append("stride")
    if any(not pos[d, j % N] for d in range(case.B) for j in csr.list_of(d) if not 0 <= j < N):
        m.append("wrap")
    first = {}
    if any(first.setdefault(csr.slot[d], d) != d and len(csr.positives(d, N)) for d in range(case.B)):
        m.append("dup")
    if ((X[:, :N] == 0) & pos).any():
        m.append("sign")
    return m


@pytest.mark.parametrize("case", bc.PATCH_CASES, ids=lambda c: c.name)
def test_patch_emulations_pass_and_mutants_fail(case):
    csr, X, v, O, z = bc.patch_operands(case)
    assert np.array_equal(v.astype(np.float64) @ O.astype(np.float64).T, z) and np.all(z * 2 == np.rint(z * 2))
    ref_x, ref_c, bound = bc.patch_reference(case, csr, X, z)
    for chains, rev in ((16, False), (8, True)):
        got_x, got_c = emu_patch(case, csr, X, z, chains, rev)
        assert np.array_equal(bits(got_x), bits(ref_x))
        assert np.all(np.abs(got_c - ref_c) <= bound), float(np.abs(got_c - ref_c).max())
    for mut in patch_mutants(case, csr, X):
        got_x, got_c = emu_patch(case, csr, X, z, mut=mut)
        assert not np.array_equal(bits(got_x), bits(ref_x)) or np.any(np.abs(got_c - ref_c) > bound), \
            f"mutant {mut} survives {case.name}"
        if mut != "sign":           # these move an element of X as well as the sum
            assert not np.array_equal(bits(got_x), bits(ref_x))
        else:
            assert np.any(np.abs(got_c - ref_c) > bound)


# ---------------------------------------------------------------------------------------------- fused -----
def host_scores(case):
    v, O = bc.fused_operands(case)
    z = v.astype(np.float64) @ O.astype(np.float64).T
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def emu_fused(P, t0, mut=None, by_rows=True):
    xv = (P - t0).astype(np.float32)
    x = np.where(xv == 0.0, F32(0) if mut == "marker" else bc.DENORM_MIN, xv)
    plus, minus = (F32(-0.0), F32(0.0)) if mut == "sign" else (F32(0.0), F32(-0.0))
    x = np.where(P == 1.0, plus, np.where(P == 0.0, minus, x)).astype(np.float32)
    term = t0 * clog32(P) + (bc.F1 - t0) * clog32(bc.F1 - P)              # split_clog: a normal p has the same bits
    t = term if by_rows else term.T
    acc = np.zeros(t.shape[1], dtype=np.float32)
    total = 0.0
    for a in range(t.shape[0]):                                            # 16 terms per fp32 chain, then float64
        acc += t[a]
        if a % 16 == 15 or a == t.shape[0] - 1:
            total += acc.astype(np.float64).sum()
            acc[:] = 0
    return x, -total


@pytest.mark.parametrize("case", bc.FUSED_CASES, ids=lambda c: c.name)
def test_fused_emulation_passes_and_mutants_fail(case):
    P = host_scores(case)
    eps = case.eps
    if case.find_eps:
        found = bc.find_eps_for(P, case.N)
        assert found is not None
        eps = found[0]
    t0 = bc.constants(case.N, eps)[0]
    ref_x = bc.fused_x_reference(P, t0)
    ref, mag = bc.negatives_reference(P, case.N, eps)
    bound = 32 * bc.U * mag + case.B * case.N * 2.0 ** -23
    for by_rows in (True, False):
        x, total = emu_fused(P, t0, by_rows=by_rows)
        assert np.array_equal(bits(x), bits(ref_x)) and abs(total - ref) <= bound
    if ((P == 1.0) | (P == 0.0)).any():
        assert not np.array_equal(bits(emu_fused(P, t0, "sign")[0]), bits(ref_x))
    if case.find_eps:
        assert (P == t0).any() and (bits(ref_x) == 1).any()
        assert not np.array_equal(bits(emu_fused(P, t0, "marker")[0]), bits(ref_x))


def test_find_eps_on_the_values_the_method_was_tried_with():
    """N = 3003: a +-6 ulp search around p N finds a float32 eps for 3.1e-4 and 7.7e-7, none for 1.2345e-5."""
    got = [bc.find_eps_for(np.array([p], dtype=np.float32), 3003) for p in (3.1e-4, 7.7e-7, 1.2345e-5)]
    for g in got[:2]:
        assert g is not None and F32(g[0]) / F32(3003) == g[1]
    print("\n[find_eps]", got)


# ---------------------------------------------------------------------------------------------- lists -----
def test_lists_cover_the_branches():
    names = [c.name for c in bc.ROWS_CASES + bc.GRAD_CASES + bc.PATCH_CASES + bc.FUSED_CASES]
    assert len(names) == len(set(names))
    r = bc.ROWS_CASES
    assert {c.N for c in r} >= {1, 255, 257, 1792, 1793, 2048, 2049, 5889}
    assert {c.pad == 0 for c in r} == {True, False}
    assert {n for c in r for n in c.lengths} >= {0, 1, 255, 256, 257, 600}
    assert {c.B for c in r} >= {1, 3, 70} and {c.eps for c in r} == {0.0, 0.1}
    g = bc.GRAD_CASES
    assert {c.N % 4 for c in g if grad_is_vec(c)} == {0, 1, 2, 3}
    assert any(c.ld % 2 == 1 for c in g) and any(c.off == 1 and c.ld % 4 == 0 for c in g)
    assert {c.N for c in g} >= {4096, 4097, 270339} and 270339 > 64 * 4096
    assert next(c for c in g if c.N == 270339).B == 2
    assert {n for c in g for n in c.lengths} >= {0, 1, 63, 64, 65, 200}
    p = bc.PATCH_CASES
    assert {c.c for c in p} == {1, 63, 64, 65, 200, 512}
    assert {n for c in p for n in c.lengths} >= {0, 1, 3, 4, 5, 15, 16, 17, 33, 300}
    f = bc.FUSED_CASES
    assert {c.B for c in f} >= {1, 31, 33, 70} and {c.N for c in f} >= {1, 127, 129, 3003}
    assert {c.c for c in f} >= {4, 31, 36, 200, 224, 272, 512}
    big = next(c for c in f if c.N == 5120)
    assert big.B == 448 and -(-big.N // 128) * -(-big.B // 32) == 560
    assert any(c.pad for c in f) and any(c.find_eps for c in f)


def test_every_mutant_applies_somewhere_and_planted_values_arrive():
    seen_r, seen_g, seen_p = set(), set(), set()
    for case in bc.ROWS_CASES:
        csr, P, pos, *_ = rows_setup(case)
        seen_r |= set(rows_mutants(case, csr, P, pos))
        assert np.isnan(P[:, case.N:]).all()
    assert seen_r == {"stride", "tail", "wrap", "dup", "flush"}
    planted_pos, planted_neg = set(), set()
    for case in bc.GRAD_CASES:
        csr, P, pos, _ = grad_setup(case)
        seen_g |= set(grad_mutants(case, csr, P, pos))
        if case.eps:
            t0, dt = bc.constants(case.N, case.eps)
            for val in [F32(x) for x in bc.PLANTED] + [t0, dt]:
                if ((P[:, :case.N] == val) & pos).any():
                    planted_pos.add(float(val) if val not in (t0, dt) else ("t0" if val == t0 else "dt"))
                if ((P[:, :case.N] == val) & ~pos).any():
                    planted_neg.add(float(val) if val not in (t0, dt) else ("t0" if val == t0 else "dt"))
    assert seen_g == {"unsat", "stride", "tail", "wrap", "dup", "dt_zero"}
    want = {float(F32(x)) for x in bc.PLANTED} | {"t0", "dt"}
    assert planted_pos == want and planted_neg == want
    for case in bc.PATCH_CASES:
        csr, X, *_ = bc.patch_operands(case)
        seen_p |= set(patch_mutants(case, csr, X))
    assert seen_p == {"stride", "wrap", "dup", "sign"}
