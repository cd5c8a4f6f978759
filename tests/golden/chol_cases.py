"""The float64 Gram-factor kernel (``rtk_gram_factor_f64``, csrc/rtk_chol.hip): cases, an extended-precision reference,
a float64 model of the kernel's blocked form, and the residuals the tests bound.

The operation, as the kernel's header states it.  S (k x k, symmetric, only the lower triangle is read), with
``tr = trace S``, ``D = sqrt(diag S)`` (``D_i = 1`` where the diagonal is not positive or ``equil`` is off) and
``shift = shift_diag + shift_trace tr``:

    A = D^-1 S D^-1 + shift I = L L^T,     R = L^T D,     X = D^-1 L^-T      (both upper triangular)

by a column sweep in which a pivot below ``floor_c = max(1e-14 |a_cc|, shift / 2) + 1e-300`` (a_cc: the diagonal entry
of A before the sweep) is replaced by that floor; the same row operations applied to an identity give ``T = L^-1``.
``tr <= 0`` or a non-finite value on or below the diagonal: both outputs are zero.

  * ``truth``      that algorithm, unblocked, in extended precision (``np.longdouble`` where it has a 64-bit mantissa,
                   else 40-digit ``mpmath``); ``hp="float64"`` runs the same sweep in float64;
  * ``model64``    the kernel's blocked form in float64: every 32-wide diagonal block is factored together with its
                   explicit inverse T11, the block's rows of the inverse are ``T11 @ B``, the panel is ``A21 @ T11^T``
                   and the trailing updates use the panel.  It is the peer for what has no derived bound (the explicit
                   block inverse), and the carrier of the mutants;
  * ``residuals``  componentwise normalised residuals of ``A - L L^T``, ``L T - I`` and ``T L - I`` with
                   ``L^T = R D^-1`` and ``T^T = D X``; A and D are formed in extended precision, so forming A in float64
                   is part of what is measured.

Bounds (u = 2^-53), with where they come from:

  B1  rho_L  <= (k + 1) u + 8 u.  (k + 1) u is the componentwise backward error of Cholesky (Higham, Accuracy and
      Stability of Numerical Algorithms, Theorem 10.3), which holds for any order of summation and with FMA; 8 u
      covers forming A in float64 (one reciprocal, two products, one add, the rounded D on both sides of R) and a pivot
      and reciprocal that come from rsq + Newton steps and not from correctly rounded operations.
  B2  rho_LT, rho_TL <= 4 max((k + 1) u, model64's value on the same case): the explicit block inverse has no clean
      derived bound, so the number comes from the model; 4 covers another order inside the 32-term sums.
  B3  max |R - R*| / max |R*| and the same for X  <= 4 (model64's own error) + 4 u   (``plain`` and ``scaled``).

Host-only (numpy; mpmath only where longdouble is a double).
"""
import functools
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -53
NB, KMAX, NT, IB = 32, 256, 1024, 8         # block width, largest k, threads, loads in flight (csrc/rtk_chol.hip)

# no skip where longdouble is a double: the reference is then 40-digit mpmath (slower, the same figures)
EXTENDED = "longdouble" if np.finfo(np.longdouble).eps < 1e-18 else "mpmath"
assert EXTENDED == "mpmath" or np.finfo(np.longdouble).eps < 1e-18


def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath

SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 96, 129, 200, 255, 256)
FAMILIES = ("plain", "scaled", "illcond")
MODES = ((0, 0.0, 0.0), (1, 1e-13, 0.0), (0, 0.0, 1e-3), (1, 3e-6, 0.0))     # (equil, shift_diag, shift_trace)

LABELS = frozenset({
    # the blocked sweep
    "only_block_partial", "only_block_full", "last_block_partial", "last_block_full", "k1",
    "below_0", "below_15", "below_16", "below_17", "nlt_max", "nbt_max", "ntri_below_waves", "ntri_above_waves",
    "copyin_last_partial", "copyin_last_full", "copyin_several",
    # modes and families
    "equil", "no_equil", "shift_diag", "shift_trace", "no_shift", "plain", "scaled", "illcond",
    # the floor path and the contract's edges
    "floor_first_block", "floor_second_block", "floor_f32_gram", "zero_column_first_block",
    "zero_column_second_block", "nonfinite_lower", "nonfinite_diag", "nonfinite_upper_ignored",
})


@dataclass(frozen=True)
class CholCase:
    """kind: grid | dup (column col duplicates col - 1) | f32gram | zerocol (column col is zero) | plant (value planted
    at ``at``).  floored: the columns whose pivot the reference floors."""
    name: str
    family: str
    k: int
    mode: tuple
    kind: str = "grid"
    col: int = -1
    at: tuple = ()
    value: float = 0.0
    floored: tuple = ()


# The floored columns of the f32gram case.  Every pivot of that case is at least 15 % away from its floor (the host
# test asserts 5 %), so rounding cannot move a column into or out of the set.
F32_FLOORED = (42, 44, 46, 51, 56)


def _cases():
    out = []
    for fam in FAMILIES:
        for k in SIZES:
            for m, mode in enumerate(MODES):
                out.append(CholCase(f"{fam}-k{k}-m{m}", fam, k, mode))
    out.append(CholCase("dup-k24-c5", "plain", 24, MODES[0], kind="dup", col=5, floored=(5,)))
    out.append(CholCase("dup-k80-c37", "plain", 80, MODES[0], kind="dup", col=37, floored=(37,)))
    out.append(CholCase("f32gram-k60", "plain", 60, MODES[3], kind="f32gram", floored=F32_FLOORED))
    for col in (20, 33):
        for m in (1, 3):
            out.append(CholCase(f"zerocol-k40-c{col}-m{m}", "scaled", 40, MODES[m], kind="zerocol", col=col))
    out.append(CholCase("nan-lower-k40", "plain", 40, MODES[1], kind="plant", at=(7, 5), value=float("nan")))
    out.append(CholCase("inf-diag-k40", "plain", 40, MODES[1], kind="plant", at=(3, 3), value=float("inf")))
    out.append(CholCase("nan-upper-k40", "plain", 40, MODES[1], kind="plant", at=(5, 7), value=float("nan")))
    return tuple(out)


def features(case):
    """The branches of the kernel (and of the contract) that a case reaches."""
    k, f = case.k, set()
    nblocks = -(-k // NB)
    if nblocks == 1:
        f.add("only_block_partial" if k < NB else "only_block_full")
    f.add("last_block_partial" if k % NB else "last_block_full")
    if k == 1:
        f.add("k1")
    for j0 in range(0, k, NB):
        w = min(NB, k - j0)
        below, left = k - j0 - w, j0 + w
        if below in (0, 15, 16, 17):
            f.add(f"below_{below}")
        nlt, nbt = (left + 15) >> 4, (below + 15) >> 4
        if nlt == KMAX // 16:
            f.add("nlt_max")
        if nbt == (KMAX - NB) // 16:
            f.add("nbt_max")
        ntri = nbt * (nbt + 1) // 2
        if 0 < ntri < 16:
            f.add("ntri_below_waves")
        if ntri > 16:
            f.add("ntri_above_waves")
    f.add("copyin_last_partial" if (k * k) % (IB * NT) else "copyin_last_full")
    if k * k > IB * NT:
        f.add("copyin_several")
    equil, sd, st = case.mode
    f.add("equil" if equil else "no_equil")
    f.add("shift_diag" if sd > 0 else "shift_trace" if st > 0 else "no_shift")
    if case.kind == "grid":
        f.add(case.family)
    if case.kind == "dup":
        f.add("floor_first_block" if case.col < NB else "floor_second_block")
    if case.kind == "f32gram":
        f.add("floor_f32_gram")
    if case.kind == "zerocol":
        f.add("zero_column_first_block" if case.col < NB else "zero_column_second_block")
    if case.kind == "plant":
        i, j = case.at
        f.add("nonfinite_diag" if i == j else "nonfinite_lower" if i > j else "nonfinite_upper_ignored")
    return f


# ------------------------------------------------------------------------------------------------ matrices


@functools.lru_cache(maxsize=None)
def factor_w(family, k, seed=None):
    """W ((2k + 3) x k) of a family, seeded by k (or ``seed``); read-only, computed once."""
    rng = np.random.default_rng(k if seed is None else seed)
    n = 2 * k + 3
    if family == "plain":
        w = rng.standard_normal((n, k))
    elif family == "scaled":
        w = rng.standard_normal((n, k)) * np.logspace(0, -4, k)
    elif family == "illcond":            # equilibrated condition number 1e8
        q = np.linalg.qr(rng.standard_normal((n, k)))[0]
        o = np.linalg.qr(rng.standard_normal((k, k)))[0]
        w = (q * np.logspace(0, -4, k)) @ o
    else:
        raise ValueError(family)
    w.setflags(write=False)
    return w


def _f32_gram(k=60, n=10000, base=40):
    """A float32-accumulated Gram matrix of dependent columns: 40 independent columns and 20 small-integer
    combinations of two of them, scaled by powers of two; every entry is ONE sequential float32 sum of float32
    products (elementwise IEEE operations only, so the matrix does not depend on a BLAS).  Its rounding noise is about
    one shift of 3e-6 on the equilibrated matrix: some pivots of the dependent columns fall below half the shift, none
    so far below that the entries behind a floored pivot grow (the noise stays under the floor)."""
    rng = np.random.default_rng(6060)
    b = rng.standard_normal((n, base))
    w = np.empty((n, k))
    w[:, :base] = b
    for j in range(base, k):
        p, q = (3 * j) % base, (7 * j + 1) % base
        w[:, j] = (1 + j % 3) * b[:, p] - (1 + j % 2) * b[:, q if q != p else (q + 1) % base]
    w = (w * 2.0 ** -(np.arange(k) % 13)).astype(np.float32)
    s = np.empty((k, k), dtype=np.float32)
    for i in range(k):
        s[i] = np.cumsum(w[:, i:i + 1] * w, axis=0, dtype=np.float32)[-1]
    return s.astype(np.float64), w.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _matrix(case):
    if case.kind == "f32gram":
        s, w = _f32_gram(case.k)
    else:
        w = factor_w(case.family, case.k).copy()
        if case.kind == "dup":
            w[:, case.col] = w[:, case.col - 1]
        if case.kind == "zerocol":
            w[:, case.col] = 0.0
        s = w.T @ w
        s = np.tril(s) + np.tril(s, -1).T
        if case.kind == "plant":
            s[case.at] = case.value
    s.setflags(write=False)
    w.setflags(write=False)
    return s, w


def matrix(case):
    """S (k x k float64, read-only) of a case."""
    return _matrix(case)[0]


def factor(case):
    """The W of a case (S = W^T W up to the case's planted entry / its float32 accumulation)."""
    return _matrix(case)[1]


def clean(case):
    """The case without its planted value."""
    return CholCase(case.name + "-clean", case.family, case.k, case.mode)


# ------------------------------------------------------------------------------------------------ extended precision


def _hp(a, hp):
    a = np.asarray(a)
    if hp == "float64":
        return np.array(a, dtype=np.float64)
    if hp == "longdouble":
        return np.array(a, dtype=np.longdouble)
    if a.dtype == object:
        return a.copy()
    return np.vectorize(_mp().mpf, otypes=[object])(np.asarray(a, dtype=np.float64))


def _sqrt(a, hp):
    if hp == "mpmath":
        return np.vectorize(_mp().sqrt, otypes=[object])(a)
    return np.sqrt(a)


def _f64(a):
    return np.asarray(a).astype(np.float64)


def lower_is_finite(S):
    return bool(np.isfinite(np.tril(np.asarray(S, dtype=np.float64))).all())


@dataclass
class Scaled:
    A: object           # the scaled, shifted matrix (symmetric, from the lower triangle of S)
    D: object
    shift: object
    floor: object       # per column


def scaled(S, equil, shift_diag, shift_trace, hp=EXTENDED):
    """A = D^-1 S D^-1 + shift I with its D, shift and pivot floors in precision ``hp``; None where the outputs are
    zero (trace <= 0 or a non-finite value on or below the diagonal)."""
    S = np.asarray(S, dtype=np.float64)
    k = S.shape[0]
    if not lower_is_finite(S):
        return None
    low = np.tril(S)
    Sx = _hp(low + np.tril(low, -1).T, hp)
    diag = Sx.diagonal().copy()
    tr = diag.sum()
    if not tr > 0:
        return None
    one = _hp(1.0, hp)[()]
    D = np.full(k, one, dtype=Sx.dtype)
    if equil:
        d = _sqrt(np.where(diag > 0, diag, 0 * diag), hp)
        D = np.where(d > 0, d, D)
    shift = _hp(shift_diag, hp)[()] + _hp(shift_trace, hp)[()] * tr
    A = Sx / (D[:, None] * D[None, :])
    idx = np.arange(k)
    A[idx, idx] = A[idx, idx] + shift
    dg = abs(A.diagonal())
    floor = np.where(_hp(1e-14, hp)[()] * dg > shift / 2, _hp(1e-14, hp)[()] * dg, shift / 2 + 0 * dg) + _hp(1e-300, hp)[()]
    return Scaled(A, D, shift, floor)


def truth(S, equil, shift_diag, shift_trace, hp=EXTENDED):
    """(R, X, floored columns) by the unblocked column sweep in precision ``hp`` (arrays of that precision)."""
    k = np.asarray(S).shape[0]
    sc = scaled(S, equil, shift_diag, shift_trace, hp)
    if sc is None:
        z = _hp(np.zeros((k, k)), hp)
        return z, z.copy(), []
    A, D = sc.A.copy(), sc.D
    L = _hp(np.zeros((k, k)), hp)
    T = _hp(np.eye(k), hp)
    floored = []
    for c in range(k):
        x = A[c, c]
        if x < sc.floor[c]:
            x = sc.floor[c]
            floored.append(c)
        piv = _sqrt(np.array([x], dtype=A.dtype), hp)[0]
        L[c, c] = piv
        T[c, :c + 1] = T[c, :c + 1] / piv
        if c + 1 < k:
            l = A[c + 1:, c] / piv
            L[c + 1:, c] = l
            A[c + 1:, c + 1:] = A[c + 1:, c + 1:] - l[:, None] * l[None, :]
            T[c + 1:, :c + 1] = T[c + 1:, :c + 1] - l[:, None] * T[c, :c + 1][None, :]
    return L.T * D[None, :], T.T / D[:, None], floored


MUTANTS = ("newton", "tile_skip", "left_minus_1", "d_wrong_side", "unzeroed", "floor_rel_only")


def model64(S, equil, shift_diag, shift_trace, mutant=None):
    """(R, X, floored columns) by the kernel's blocked form in float64.  ``mutant``: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    S = np.asarray(S, dtype=np.float64)
    k = S.shape[0]
    zero = (np.zeros((k, k)), np.zeros((k, k)), [])
    if not lower_is_finite(S):
        return zero
    diag = S.diagonal().copy()
    tr = diag.sum()
    if not tr > 0.0:
        return zero
    d = np.sqrt(np.maximum(diag, 0.0))
    on = (d > 0.0) & bool(equil)
    dsc = np.where(on, d, 1.0)
    idsc = np.where(on, 1.0 / np.where(on, d, 1.0), 1.0)
    shift = shift_diag + shift_trace * tr
    Lo = np.tril((S * idsc[:, None]) * idsc[None, :])
    idx = np.arange(k)
    Lo[idx, idx] += shift
    Ti = np.eye(k)
    dg = Lo.diagonal().copy()
    floored = []
    for j0 in range(0, k, NB):
        w = min(NB, k - j0)
        below, left = k - j0 - w, j0 + w
        # A) the diagonal block with its explicit inverse
        blk = np.tril(Lo[j0:left, j0:left])
        t11 = np.eye(w)
        for c in range(w):
            floor = max(1e-14 * abs(dg[j0 + c]), 0.0 if mutant == "floor_rel_only" else 0.5 * shift) + 1e-300
            x = blk[c, c]
            if not x >= floor:
                x = floor
                floored.append(j0 + c)
            ip = 1.0 / np.sqrt(x)
            if mutant == "newton":
                ip *= 1.0 + 2.0 ** -40
            piv = np.sqrt(x)
            col = blk[:, c] * ip
            trow = t11[c, :c + 1] * ip
            blk[c, c] = piv
            blk[c + 1:, c] = col[c + 1:]
            t11[c, :c + 1] = trow
            if c + 1 < w:
                blk[c + 1:, c + 1:] -= np.tril(np.outer(col[c + 1:], col[c + 1:]))
                t11[c + 1:, :c + 1] -= np.outer(col[c + 1:], trow)
        Lo[j0:left, j0:left] = blk
        # A2) the block's rows of the inverse
        B = Ti[j0:left, :left].copy()
        live = left - 1 if mutant == "left_minus_1" else left
        B[:, :live] = t11 @ B[:, :live]
        Ti[j0:left, :left] = B
        if below:
            # B) the panel
            pan = Lo[left:, j0:left] @ t11.T
            Lo[left:, j0:left] = pan
            # C) trailing updates, in 16-row tiles
            upd = np.tril(pan @ pan.T)
            if mutant == "tile_skip" and below % 16:
                upd[below - below % 16:] = 0.0
            Lo[left:, left:] -= upd
            Ti[left:, :left] -= pan @ B
    if mutant == "d_wrong_side":
        X = Ti.T * idsc[None, :]
    else:
        X = Ti.T * idsc[:, None]
    R = Lo.T * dsc[None, :]
    if mutant != "unzeroed":
        R, X = np.triu(R), np.triu(X)
    else:
        R, X = np.triu(R) + np.tril(Lo, -1), np.triu(X) + np.tril(Ti, -1)
    return R, X, floored


# ------------------------------------------------------------------------------------------------ what the tests measure


def _ratio(num, den):
    """max over the lower triangle of num / den; 0 / 0 counts as 0, x / 0 as inf."""
    num, den = np.tril(_f64(num)), np.tril(den)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
    return float(r.max())


def residuals(S, R, X, equil, shift_diag, shift_trace, hp=EXTENDED):
    """dict(rho_L, rho_LT, rho_TL): the componentwise normalised residuals of A - L L^T, L T - I and T L - I on the
    lower triangle, with L^T = R D^-1 and T^T = D X; products in extended precision, normalisers in float64."""
    sc = scaled(S, equil, shift_diag, shift_trace, hp)
    assert sc is not None
    k = sc.D.shape[0]
    Lt = _hp(R, hp) / sc.D[None, :]
    Tt = sc.D[:, None] * _hp(X, hp)
    L, T = Lt.T, Tt.T
    aL, aT = np.abs(_f64(L)), np.abs(_f64(T))
    eye = _hp(np.eye(k), hp)
    return dict(rho_L=_ratio(abs(sc.A - L @ Lt), aL @ aL.T),
                rho_LT=_ratio(abs(L @ T - eye), aL @ aT),
                rho_TL=_ratio(abs(T @ L - eye), aT @ aL))


def forward_error(got, ref, hp=EXTENDED):
    """max |got - ref| / max |ref|."""
    ref = _hp(ref, hp)
    den = abs(ref).max()
    return float(abs(_hp(got, hp) - ref).max() / den) if den > 0 else float(abs(_hp(got, hp)).max())


def bound_L(k):
    return (k + 1) * U + 8 * U


def bound_inverse(k, model_rho):
    return 4.0 * max((k + 1) * U, model_rho)


def bound_forward(model_err):
    return 4.0 * model_err + 4 * U


def exact_properties(S, R, X, equil, shift_diag, shift_trace, hp=EXTENDED):
    """B4, the part that needs no device: a list of what is wrong (empty = fine) -- every element finite, the strict
    lower triangles exactly zero, and R[i, i] / D_i >= sqrt(floor_i) (1 - 4 u)."""
    bad = []
    R, X = np.asarray(R, dtype=np.float64), np.asarray(X, dtype=np.float64)
    if not (np.isfinite(R).all() and np.isfinite(X).all()):
        bad.append("a non-finite element")
    if np.tril(R, -1).view(np.uint64).any() or np.tril(X, -1).view(np.uint64).any():
        bad.append("the strict lower triangle is not +0")
    sc = scaled(S, equil, shift_diag, shift_trace, hp)
    if sc is None:
        if R.view(np.uint64).any() or X.view(np.uint64).any():
            bad.append("outputs of a dead matrix are not +0")
        return bad
    low = _f64(_sqrt(sc.floor, hp) * sc.D) * (1 - 4 * U)
    if not (R.diagonal() >= low).all():
        i = int(np.argmin(R.diagonal() - low))
        bad.append(f"pivot {i} below its floor: {R[i, i]!r} < {low[i]!r}")
    return bad


@dataclass
class Reference:
    R: object           # extended precision
    X: object
    floored: list
    model: tuple        # (R, X, floored) of model64
    model_rho: dict     # residuals of the model (None where a pivot is floored)
    model_fwd: tuple    # forward errors of the model's R, X against the truth


@functools.lru_cache(maxsize=None)
def reference(case):
    """truth and model64 of a case with the model's own figures: computed once, shared by the tests, never changed."""
    S = matrix(case)
    R, X, floored = truth(S, *case.mode)
    model = model64(S, *case.mode)
    live = scaled(S, *case.mode) is not None
    rho = residuals(S, model[0], model[1], *case.mode) if live and not floored else None
    fwd = (forward_error(model[0], R), forward_error(model[1], X))
    for a in (R, X, model[0], model[1]):
        a.setflags(write=False)
    return Reference(R, X, floored, model, rho, fwd)


def measure(case, R, X, rho=None):
    """dict of (value, bound) per check of a case without a floored pivot: B1, B2 and (plain, scaled) B3.  ``rho``:
    the residuals of (R, X) where they are known already."""
    ref = reference(case)
    S, k = matrix(case), case.k
    rho = residuals(S, R, X, *case.mode) if rho is None else rho
    out = dict(rho_L=(rho["rho_L"], bound_L(k)),
               rho_LT=(rho["rho_LT"], bound_inverse(k, ref.model_rho["rho_LT"])),
               rho_TL=(rho["rho_TL"], bound_inverse(k, ref.model_rho["rho_TL"])))
    if case.family in ("plain", "scaled"):
        out["fwd_R"] = (forward_error(R, ref.R), bound_forward(ref.model_fwd[0]))
        out["fwd_X"] = (forward_error(X, ref.X), bound_forward(ref.model_fwd[1]))
    return out


def floor_figures(case, R, X):
    """dict of (value, bound) for a case with floored pivots: the leading c x c blocks (c = the first floored column;
    nothing before it is touched) against B3, R[c, c] = sqrt(floor_c) D_c to 4 u for every floored c, and
    max |X| <= 4 max |model64's X|.  Entries behind a floored pivot are input noise divided by sqrt(floor): they are
    not compared element by element."""
    ref = reference(case)
    sc = scaled(matrix(case), *case.mode)
    c0 = min(case.floored)
    mR, mX = ref.model[0], ref.model[1]
    out = dict(lead_R=(forward_error(R[:c0, :c0], ref.R[:c0, :c0]),
                       bound_forward(forward_error(mR[:c0, :c0], ref.R[:c0, :c0]))),
               lead_X=(forward_error(X[:c0, :c0], ref.X[:c0, :c0]),
                       bound_forward(forward_error(mX[:c0, :c0], ref.X[:c0, :c0]))),
               max_X=(float(np.abs(X).max()), 4.0 * float(np.abs(mX).max())))
    for c in case.floored:
        want = _sqrt(sc.floor[c:c + 1], EXTENDED)[0] * sc.D[c]
        out[f"pivot_{c}"] = (float(abs(_hp(R[c, c], EXTENDED)[()] - want) / want), 4 * U)
    return out


def check(case, R, X, rho=None):
    """-> (what is wrong: a list of strings, empty = fine;  the figures: name -> (value, bound)).  Everything that
    can be said about the outputs of a case without the device: B1 - B3 (or the floor path's figures), B4's exact
    properties, a zero column that stays zero."""
    S = matrix(case)
    R, X = np.asarray(R, dtype=np.float64), np.asarray(X, dtype=np.float64)
    bad = exact_properties(S, R, X, *case.mode)
    if bad or scaled(S, *case.mode) is None:
        return bad, {}
    figures = floor_figures(case, R, X) if case.floored else measure(case, R, X, rho)
    bad += [f"{n} = {v:.3e} > {b:.3e}" for n, (v, b) in figures.items() if not v <= b]
    if case.kind == "zerocol":
        c = case.col
        Q = factor(case) @ X
        if np.abs(Q[:, c]).max() != 0 or np.abs(X[:c, c]).max() != 0 or np.abs(R[c, c + 1:]).max() != 0:
            bad.append(f"the zero column {c} does not stay zero")
    return bad, figures


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
GRID = tuple(c for c in CASES if c.kind == "grid")
FLOOR = tuple(c for c in CASES if c.kind in ("dup", "f32gram"))
ZEROCOL = tuple(c for c in CASES if c.kind == "zerocol")
PLANTED = tuple(c for c in CASES if c.kind == "plant")
