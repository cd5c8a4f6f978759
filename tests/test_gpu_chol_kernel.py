"""rtk_gram_factor_f64 (csrc/rtk_chol.hip) through its C ABI, to rounding level on every branch: residual bounds
against the extended-precision sweep of tests/golden/chol_cases.py (B1 derived, B2 / B3 against the float64 model of
the kernel's blocked form), exact properties of the outputs, and bit equality between the kernel and itself (batches,
repeated launches).  No emulation of the kernel's bits: the pivot comes from v_rsq_f64.

Every launch: both outputs pre-filled with NaN, 64 doubles of a sentinel behind each, S compared with itself
afterwards.  tests/test_chol_cases_host.py proves the cases, the caps and the mutants on the host.
"""
import numpy as np
import pytest
import torch

import chol_cases as cc

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.0e30
by_name = dict(ids=lambda c: c.name)
WORST = {}            # kind of bound -> (value / bound, case): what test_report_worst_ratios prints


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def out_buffer(n):
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    buf[n:] = SENTINEL
    return buf


def launch(lib, S, mode, expect=0, k=None, batch=None, ptrs=None):
    """One launch on S (nb, k, k) -> (R, X) as the kernel left them (numpy); checks the guards and S.  ``expect`` != 0:
    the call has to return that status and leave both outputs as they were.  ``ptrs``: maps the (S, R, X) device
    pointers to the ones passed (argument checks)."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    S = S.reshape((-1,) + S.shape[-2:])
    nb, kk = S.shape[0], S.shape[-1]
    n = nb * kk * kk
    d_S = torch.from_numpy(S.copy()).cuda()
    bR, bX = out_buffer(n), out_buffer(n)
    before = bR.cpu().numpy()
    p = (d_S.data_ptr(), bR.data_ptr(), bX.data_ptr())
    p = p if ptrs is None else ptrs(*p)
    equil, sd, st = mode
    rc = lib.rtk_gram_factor_f64(p[0], nb if batch is None else batch, kk if k is None else k, int(equil), float(sd),
                                 float(st), p[1], p[2], torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, lib.rtk_last_error_string())
    torch.cuda.synchronize()
    hR, hX = bR.cpu().numpy(), bX.cpu().numpy()
    assert np.array_equal(bits(d_S.cpu().numpy()), bits(S)), "S was written"
    for h, what in ((hR, "R"), (hX, "X")):
        assert np.array_equal(bits(h[n:]), bits(before[n:])), f"written past {what}"
        if expect:
            assert np.array_equal(bits(h), bits(before)), f"{what} touched by a refused call"
    return hR[:n].reshape(S.shape), hX[:n].reshape(S.shape)


def note(kind, value, bound, name):
    ratio = value / bound if bound > 0 else float("inf")
    if ratio > WORST.get(kind, (-1.0, ""))[0]:
        WORST[kind] = (ratio, name)


def pivot_errors(case, R):
    """Relative errors of the kernel's pivots (the diagonal of L) against the extended sweep: what a miss of a bound
    on a run that otherwise looks right would be about."""
    ref = cc.reference(case)
    want = cc._f64(ref.R.diagonal())
    return float(np.abs((R.diagonal() - want) / want).max())


@pytest.mark.parametrize("case", cc.GRID + cc.ZEROCOL + cc.FLOOR, **by_name)
def test_outputs_to_rounding_level(lib, case):
    """B1 - B4 (a floor case: the floor path's figures of section C), one one-workgroup launch per case."""
    S = cc.matrix(case)
    R, X = launch(lib, S, case.mode)
    R, X = R[0], X[0]
    bad, fig = cc.check(case, R, X)
    line = "  ".join(f"{n} {v / b:.3f}" for n, (v, b) in fig.items())
    print(f"\n[{case.name}] value / bound: {line}")
    for n, (v, b) in fig.items():
        note({"rho_L": "B1 rho_L", "rho_LT": "B2 rho_LT / rho_TL", "rho_TL": "B2 rho_LT / rho_TL",
              "fwd_R": "B3 forward R / X", "fwd_X": "B3 forward R / X"}.get(n, "floor path " + n.split("_")[0]), v, b, case.name)
    assert not bad, f"[{case.name}] " + "; ".join(bad) + f"; max relative pivot error {pivot_errors(case, R):.3e}"
    if case.floored:                                    # the kernel floors what the reference floors
        sc = cc.scaled(S, *case.mode)
        at_floor = np.abs(R.diagonal() / (np.sqrt(cc._f64(sc.floor)) * cc._f64(sc.D)) - 1) <= 1e-6   # the others: > 2 % above
        assert sorted(np.flatnonzero(at_floor)) == list(case.floored)


def test_report_worst_ratios():
    """The worst value / bound of each kind over the cases above (DESIGN.md section 8 records them)."""
    for kind in sorted(WORST):
        print(f"\nworst {kind}: {WORST[kind][0]:.3f} of its bound at {WORST[kind][1]}")
    assert all(r <= 1.0 for r, _ in WORST.values())


def neighbours(k, seeds):
    return [np.asarray(cc.factor_w("plain", k, seed=s).T @ cc.factor_w("plain", k, seed=s)) for s in seeds]


@pytest.mark.parametrize("case", cc.PLANTED, **by_name)
def test_non_finite_input(lib, case):
    """C2: a non-finite value on or below the diagonal gives zero R and X; above the diagonal nothing is read (the
    bits of the clean matrix).  Inside a batch whose neighbours keep their bits."""
    k = case.k
    a, b = neighbours(k, (7001, 7002))
    R, X = launch(lib, np.stack([a, cc.matrix(case), b]), case.mode)
    for i, m in ((0, a), (2, b)):
        R1, X1 = launch(lib, m, case.mode)
        assert np.array_equal(bits(R[i]), bits(R1[0])) and np.array_equal(bits(X[i]), bits(X1[0])), f"neighbour {i}"
        assert np.isfinite(R[i]).all() and np.isfinite(X[i]).all()
    i, j = case.at
    if i >= j:
        assert not bits(R[1]).any() and not bits(X[1]).any(), "outputs of a non-finite matrix are not +0"
    else:
        Rc, Xc = launch(lib, cc.matrix(cc.clean(case)), case.mode)
        assert np.array_equal(bits(R[1]), bits(Rc[0])) and np.array_equal(bits(X[1]), bits(Xc[0]))
        assert np.isfinite(R[1]).all() and R[1].any()


@pytest.mark.parametrize("k", [17, 49, 200])
def test_batches_equal_single_launches(lib, k):
    """B5: five matrices in one launch = five launches, bit for bit; one of them replaced by a zero matrix gives zero
    outputs there and leaves the others' bits; a second identical launch gives identical bits."""
    mats = neighbours(k, range(9000 + k, 9005 + k))
    mode = cc.MODES[1]
    R, X = launch(lib, np.stack(mats), mode)
    for i, m in enumerate(mats):
        R1, X1 = launch(lib, m, mode)
        assert np.array_equal(bits(R[i]), bits(R1[0])) and np.array_equal(bits(X[i]), bits(X1[0])), i
        rho = cc.residuals(m, R[i], X[i], *mode) if i == 4 else None         # and they are factors (one is enough)
        assert rho is None or rho["rho_L"] <= cc.bound_L(k)
    R2, X2 = launch(lib, np.stack(mats), mode)
    assert np.array_equal(bits(R), bits(R2)) and np.array_equal(bits(X), bits(X2))
    mats[2] = np.zeros((k, k))
    Rz, Xz = launch(lib, np.stack(mats), mode)
    assert not bits(Rz[2]).any() and not bits(Xz[2]).any()
    keep = [0, 1, 3, 4]
    assert np.array_equal(bits(Rz[keep]), bits(R[keep])) and np.array_equal(bits(Xz[keep]), bits(X[keep]))


def test_argument_checks(lib):
    """B6: the statuses include/rtucker_hip.h documents; a refused call leaves both outputs untouched."""
    BAD_ARG, UNSUPPORTED = -1, -3
    S = neighbours(8, (1,))[0]
    mode = cc.MODES[1]
    for k in (0, 257):
        launch(lib, S, mode, expect=UNSUPPORTED, k=k)
    for batch in (0, 1 << 20):
        launch(lib, S, mode, expect=BAD_ARG, batch=batch)
    for null in range(3):
        launch(lib, S, mode, expect=BAD_ARG, ptrs=lambda *p, null=null: tuple(None if i == null else q for i, q in enumerate(p)))
    launch(lib, S, mode, expect=BAD_ARG, ptrs=lambda s, r, x: (s, s, x))
    launch(lib, S, mode, expect=BAD_ARG, ptrs=lambda s, r, x: (s, r, s))
    launch(lib, S, mode, expect=BAD_ARG, ptrs=lambda s, r, x: (s, r, r))
    launch(lib, S, (1, -1e-13, 0.0), expect=BAD_ARG)
    launch(lib, S, (1, 0.0, -1e-3), expect=BAD_ARG)
    R, X = launch(lib, S, mode)                          # and the same operands are taken when nothing is wrong
    assert np.isfinite(R).all() and np.isfinite(X).all()


# ------------------------------------------------------------------------------------------------ B7: the Python layer


def tbits(t):
    return bits(t.detach().cpu().numpy())


def test_gram_factor_many_equals_the_single_calls_on_the_device():
    from r_tucker_amd import smalllinalg as sl
    mats = [torch.from_numpy(neighbours(k, (60 + i,))[0]).cuda() for i, k in enumerate((5, 7, 5, 5, 7))]
    for (X, R), S in zip(sl.gram_factor_many(mats), mats):
        X1, R1 = sl.gram_factor(S)
        assert np.array_equal(tbits(X), tbits(X1)) and np.array_equal(tbits(R), tbits(R1))
        rho = cc.residuals(S.cpu().numpy(), R.cpu().numpy(), X.cpu().numpy(), *cc.MODES[1])
        assert rho["rho_L"] <= cc.bound_L(S.shape[-1])


def test_gram_factor_takes_float32_views_and_batch_dimensions():
    from r_tucker_amd import smalllinalg as sl
    k = 33
    mats = neighbours(k, range(70, 76))
    S = torch.from_numpy(mats[0]).cuda()
    X0, R0 = sl.gram_factor(S)
    # float32: factored in float64, as the float64 copy of the same numbers
    S32 = S.float()
    X, R = sl.gram_factor(S32)
    X1, R1 = sl.gram_factor(S32.double())
    assert X.dtype == torch.float64 and np.array_equal(tbits(X), tbits(X1)) and np.array_equal(tbits(R), tbits(R1))
    rho = cc.residuals(S32.double().cpu().numpy(), R.cpu().numpy(), X.cpu().numpy(), *cc.MODES[1])
    assert rho["rho_L"] <= cc.bound_L(k)
    # a transposed view: M holds S on and above its diagonal and a sentinel below, so M^T is S where S is read; a
    # layer that passed the view's storage on would factor the sentinel
    M = torch.triu(S) + torch.tril(torch.full_like(S, SENTINEL), -1)
    view = M.transpose(0, 1)
    assert not view.is_contiguous()
    X, R = sl.gram_factor(view)
    assert np.array_equal(tbits(X), tbits(X0)) and np.array_equal(tbits(R), tbits(R0))
    # leading batch dimensions
    B = torch.from_numpy(np.stack(mats).reshape(2, 3, k, k)).cuda()
    X, R = sl.gram_factor(B)
    assert X.shape == R.shape == (2, 3, k, k)
    for i in range(2):
        for j in range(3):
            X1, R1 = sl.gram_factor(B[i, j])
            assert np.array_equal(tbits(X[i, j]), tbits(X1)) and np.array_equal(tbits(R[i, j]), tbits(R1))


def test_k_257_takes_the_torch_fallback_and_meets_the_factor_bound():
    from r_tucker_amd import smalllinalg as sl
    k = 257
    assert k > sl._HIP_CHOL_MAX
    S = neighbours(k, (257,))[0]
    X, R = sl.gram_factor(torch.from_numpy(S).cuda())
    X, R = X.cpu().numpy(), R.cpu().numpy()
    assert np.isfinite(X).all() and np.isfinite(R).all() and not np.tril(R, -1).any() and not np.tril(X, -1).any()
    rho = cc.residuals(S, R, X, *cc.MODES[1])
    print(f"\nk = 257 fallback: rho_L = {rho['rho_L'] / cc.bound_L(k):.3f} of its bound")
    assert rho["rho_L"] <= cc.bound_L(k)
