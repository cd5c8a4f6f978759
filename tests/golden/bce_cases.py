"""Inputs, float64 references, bounds and case lists for the matrix-form BCE loss kernels (csrc/rtk_bce.hip and the
loss epilogue of csrc/rtk_score_split_kernel.h), driven through their four C entry points.

Every constant is formed the way the kernels form it, in fp32:
    eps32 = float32(eps),  t0 = eps32 / float32(N),  dt = float32(1) - eps32,  s = g * scale.

  CSR      unique objects per list, the list lengths of the case (an empty list among them); lists of six or more
           entries hold the out-of-range ids -1, N and N + 5 (positions 1, len // 2, len - 2), which every kernel has
           to skip; the batch rows cycle through the lists, so several rows point at the same slot.
  P        score rows for the kernels that take the matrix as an argument: the logistic of N(0, 3^2) logits, with
           the PLANTED values (and t0 and dt themselves) in positive and in negative columns; columns 0, 5 and N - 1
           stay ordinary, so an out-of-range id that a kernel wrapped would land on a score that shows.  ld > N: the
           padding is NaN.
  rows     float64 reference from the same fp32 P:  term = t0 L(p) + (1 - t0) L(1 - p), plus dt (L(p) - L(1 - p))
           on the row's unique in-range positives, L(x) = max(ln x, -100), 1 - p formed in float64.
           Bound: k 2^-24 sum|terms| + N 2^-23, k = ceil(N / 256) + ceil(L / 256) + 16 -- a lane's fp32 chain plus
           sixteen roundings per term (two logs of 1 ulp, the ln 2 scaling, products and sum, factor two of slack);
           the floor is the rounding of 1.0f - p below 1.  sum|terms| adds |t0 L(p)|, |(1 - t0) L(1 - p)|, |dt L(p)|
           and |dt L(1 - p)| separately: the roundings of a difference scale with its operands.  On top of it the
           project's cap 2e-6 max(1, |ref|) (tests/test_gpu_loss.py) holds: the asserted bound is the smaller one.
  grad     bit for bit in numpy fp32.  Pass 1: x = p - dt on unique in-range positives with p not 0.0 or 1.0.
           Pass 2: out = 0 where the SCORE was saturated, else (x - t0) s.  A positive whose score equals dt has the
           gradient -t0 s (include/rtucker_hip.h: saturated means exactly 1.0f or 0.0f).
  patch    v and O rows of small (half-)integers: every logit is exact in fp32 in any order, |z| in [0.5, 8].

Host-only (numpy).  tests/test_bce_cases_host.py proves the method without a GPU (fp32 emulations pass, mutants
fail); tests/test_gpu_bce_kernels.py parametrizes over the same lists.
"""
import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
F1 = np.float32(1)
DENORM_MIN = np.array([1], dtype=np.uint32).view(np.float32)[0]          # bits 0x00000001
PLANTED = [0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -126, 2.0 ** -127, 1e-40, 2.0 ** -149, 0.5]      # + t0 and dt of the case
KEEP_ORDINARY = (0, 5, -1)      # columns (modulo N) that out-of-range ids would wrap to


def _seed(name):
    return zlib.crc32(name.encode())


def constants(N, eps):
    """(t0, dt) as float32, formed like the kernels' hosts form them."""
    eps32 = np.float32(eps)
    return eps32 / np.float32(N), F1 - eps32


def grad_factor(g, scale):
    return np.float32(g) * np.float32(scale)


def L(x):
    """max(ln x, -100) in float64 (ln 0 = -inf -> -100)."""
    with np.errstate(divide="ignore"):
        return np.maximum(np.log(np.asarray(x, dtype=np.float64)), -100.0)


# ---------------------------------------------------------------------------------------------- CSR -------
@dataclass(frozen=True)
class Csr:
    slot: np.ndarray        # (B,) int64: list of every batch row
    ptr: np.ndarray         # (n_lists + 1,) int64
    obj: np.ndarray         # int64, out-of-range ids included

    def list_of(self, d):
        s = self.slot[d]
        return self.obj[self.ptr[s]:self.ptr[s + 1]]

    def positives(self, d, N):
        """The row's in-range objects, in list order (unique by construction)."""
        l = self.list_of(d)
        return l[(l >= 0) & (l < N)]


def build_csr(rng, N, lengths, B):
    lists = []
    for n in lengths:
        bad = {1: -1, n // 2: N, n - 2: N + 5} if n >= 6 else {}
        good = rng.permutation(N)[:min(n - len(bad), N)]
        l = good.tolist()
        for i in sorted(bad):
            l.insert(min(i, len(l)), bad[i])
        lists.append(l)
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    obj = np.asarray([x for l in lists for x in l], dtype=np.int64)
    slot = (np.arange(B) % len(lists)).astype(np.int64)
    if B >= 2:
        slot[B - 1] = slot[0]            # two rows on one slot even when B <= the number of lists
    if ptr[-1] == 0:
        obj = np.zeros(1, dtype=np.int64)        # never read (every list is empty); keeps the pointer valid
    return Csr(slot, ptr, obj)


# ---------------------------------------------------------------------------------------------- cases -----
@dataclass(frozen=True)
class RowsCase:
    """rtk_bce_rows_f32 / rtk_bce_grad_f32 on a planted P.  pad: ld - N.  off: floats P is moved off a 16-byte
    boundary (gradient: the scalar path).  sigma: standard deviation of the ordinary logits."""
    name: str
    N: int
    B: int
    lengths: tuple
    eps: float = 0.1
    pad: int = 0
    off: int = 0
    sigma: float = 3.0

    @property
    def ld(self):
        return self.N + self.pad


ROWS_CASES = [
    RowsCase("n1", 1, 3, (1, 0, 6), eps=0.1),
    RowsCase("n255_eps0", 255, 3, (255, 0, 1), eps=0.0, pad=3),
    RowsCase("n257", 257, 3, (257, 1, 0), pad=0),
    RowsCase("n1792", 1792, 1, (256,), pad=8),
    RowsCase("n1793_eps0", 1793, 3, (257, 256, 0), eps=0.0),
    RowsCase("n2048", 2048, 3, (600, 255, 0), pad=5),
    RowsCase("n2049", 2049, 70, (600, 0, 1, 255, 256, 257, 12), pad=0),
    RowsCase("n5889_pad", 5889, 3, (257, 600, 0), pad=7),
    RowsCase("n5889_eps0_b70", 5889, 70, (0, 1, 255, 256, 257, 600, 40, 12, 64), eps=0.0, pad=0),
]

# the five trial cases of the bound (N, L, logit scale): host only
BOUND_TRIALS = [
    RowsCase("trial_257", 257, 2, (5,), sigma=3.0),
    RowsCase("trial_2049", 2049, 2, (257,), sigma=8.0),
    RowsCase("trial_5889", 5889, 2, (600,), sigma=20.0),
    RowsCase("trial_1793", 1793, 2, (0,), sigma=1.0),
    RowsCase("trial_3003", 3003, 2, (64,), sigma=40.0),
]

GRAD_G = -3.0
GRAD_CASES = [
    # ld % 4 == 0 and an aligned base: the vector path and its tail, N % 4 = 0, 1, 2, 3
    RowsCase("vec_n4096", 4096, 3, (200, 0, 65)),
    RowsCase("vec_n4097", 4097, 3, (64, 1, 63), pad=3),
    RowsCase("vec_n258", 258, 3, (65, 0, 1), pad=2, eps=0.0),
    RowsCase("vec_n259", 259, 70, (0, 1, 63, 64, 65, 200, 12), pad=1),
    # the scalar path: an odd ld; an aligned ld behind a base moved by 4 bytes
    RowsCase("scalar_odd_ld", 4097, 3, (65, 200, 0)),
    RowsCase("scalar_offset_base", 4096, 3, (63, 64, 0), off=1),
    RowsCase("scalar_n1", 1, 3, (1, 0, 6)),
    # beyond 64 blocks x 4096 columns: every block of the capped grid strides twice
    RowsCase("cap_n270339", 270339, 2, (200, 65), pad=1),
]


def plant(case, csr, rng=None):
    """P (B, ld) float32 and the boolean mask of the in-range positives."""
    rng = rng or np.random.default_rng(_seed(case.name) + 1)
    N, B = case.N, case.B
    t0, dt = constants(N, case.eps)
    values = [np.float32(x) for x in PLANTED] + [t0, dt]
    z = rng.standard_normal((B, N)) * case.sigma
    P = np.full((B, case.ld), np.nan, dtype=np.float32)
    P[:, :N] = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    pos = np.zeros((B, N), dtype=bool)
    keep = {k % N for k in KEEP_ORDINARY}
    for d in range(B):
        pj = csr.positives(d, N)
        pos[d, pj] = True
        free_pos = [j for j in pj.tolist() if j not in keep or N < 8]
        free_neg = [j for j in rng.permutation(N).tolist()[:64] if not pos[d, j] and (j not in keep or N < 8)]
        for cols in (free_pos, free_neg):
            for i, j in enumerate(cols[:len(values)]):
                P[d, j] = values[(d + i) % len(values)]          # rotated: short lists still see every value
    return P, pos


def rows_reference(case, P, pos):
    """float64 row sums of the BCE terms, and sum|terms| per row."""
    N = case.N
    t0, dt = [float(x) for x in constants(N, case.eps)]
    p = P[:, :N].astype(np.float64)
    lp, lq = L(p), L(1.0 - p)
    term = t0 * lp + (1.0 - t0) * lq + np.where(pos, dt * (lp - lq), 0.0)
    mag = np.abs(t0 * lp) + np.abs((1.0 - t0) * lq) + np.where(pos, np.abs(dt * lp) + np.abs(dt * lq), 0.0)
    return -term.sum(axis=1), mag.sum(axis=1)


def rows_bound(N, longest, mag, ref, k=None, floor=None):
    """The asserted row bound: min(k u sum|terms| + floor, 2e-6 max(1, |ref|))."""
    if k is None:
        k = -(-N // 256) + -(-longest // 256) + 16
    if floor is None:
        floor = N * 2.0 ** -23
    return np.minimum(k * U * mag + floor, 2e-6 * np.maximum(1.0, np.abs(ref)))


def grad_reference(case, P, pos, g=GRAD_G, scale=None):
    """fp32, bit for bit: the (B, N) result of rtk_bce_grad_f32."""
    N = case.N
    t0, dt = constants(N, case.eps)
    s = grad_factor(g, 1.0 / (case.B * N) if scale is None else scale)
    p = P[:, :N]
    sat = (p == 0.0) | (p == 1.0)
    x = np.where(pos & ~sat, p - dt, p).astype(np.float32)
    out = np.where(sat, np.float32(0), (x - t0) * s).astype(np.float32)
    assert out.dtype == np.float32
    return out


# ---------------------------------------------------------------------------------------------- patch -----
@dataclass(frozen=True)
class PatchCase:
    """rtk_bce_patch_pos_f32: X, v and O built here."""
    name: str
    N: int
    B: int
    c: int
    lengths: tuple
    eps: float = 0.1
    pad: int = 0


PATCH_CASES = [
    PatchCase("c1", 301, 3, 1, (300, 0, 1), pad=3),
    PatchCase("c63", 97, 5, 63, (3, 4, 5, 0)),
    PatchCase("c64_eps0", 97, 5, 64, (15, 16, 17), eps=0.0, pad=1),
    PatchCase("c65", 97, 3, 65, (33, 1, 0)),
    PatchCase("c200", 311, 70, 200, (0, 1, 3, 4, 5, 15, 16, 17, 33, 300), pad=2),
    PatchCase("c512", 64, 3, 512, (17, 0, 5)),
]


def patch_operands(case):
    """-> (csr, X, v, O, z): X (B, ld) with NaN padding, z the exact logits (B, N) in float64.  Positives hold +0, -0
    (the first two of a list, one sign per row) or an ordinary value; a few non-positives hold signed zeros too."""
    rng = np.random.default_rng(_seed(case.name))
    N, B, c = case.N, case.B, case.c
    csr = build_csr(rng, N, case.lengths, B)
    support = sorted({0, c // 2, c - 1, min(64, c - 1)})
    v = np.zeros((B, c), dtype=np.float32)
    v[:, support] = rng.choice([-1.0, -0.5, 0.5, 1.0], size=(B, len(support)))
    O = rng.integers(-2, 3, size=(N, c)).astype(np.float32)
    users = {}
    for d in range(B):
        for j in csr.positives(d, N).tolist():
            users.setdefault(j, []).append(d)
    for j, ds in users.items():
        for _ in range(10000):
            O[j, support] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=len(support))
            zj = np.abs(v[ds][:, support].astype(np.float64) @ O[j, support].astype(np.float64))
            if zj.min() >= 0.5 and zj.max() <= 8.0:
                break
        else:
            raise AssertionError(f"{case.name}: no O row for entity {j}")
    z = v.astype(np.float64) @ O.astype(np.float64).T
    X = np.full((B, N + case.pad), np.nan, dtype=np.float32)
    X[:, :N] = rng.standard_normal((B, N)).astype(np.float32) * np.float32(0.3)
    X[:, :N][X[:, :N] == 0] = np.float32(0.25)
    for d in range(B):
        pj = csr.positives(d, N).tolist()
        for i, j in enumerate(pj[:2]):
            X[d, j] = np.float32(0.0) if d % 2 == 0 else np.float32(-0.0)       # one sign per row: a swap cannot cancel
        neg = [j for j in rng.permutation(N).tolist()[:8] if j not in pj][:2]
        for i, j in enumerate(neg):
            X[d, j] = np.float32(-0.0) if (d + i) % 2 == 0 else np.float32(0.0)
    return csr, X, v, O, z


def patch_reference(case, csr, X, z):
    """-> (X afterwards, fp32 bit for bit; float64 row corrections; their bounds)."""
    N = case.N
    t0, dt = constants(N, case.eps)
    out = X.copy()
    corr, bound = np.zeros(case.B), np.zeros(case.B)
    hundred = float(dt * np.float32(100))
    for d in range(case.B):
        for j in csr.positives(d, N).tolist():
            x = X[d, j]
            if x == 0.0:
                corr[d] += hundred if np.signbit(x) else -hundred          # exact: the fp32 product the kernel forms
                continue
            out[d, j] = x - dt
            zz = z[d, j]
            p = 1.0 / (1.0 + np.exp(-zz))
            corr[d] += -float(dt) * (np.log(p) - np.log1p(-p))
            bound[d] += 2.0 * float(dt) * ((2 * abs(zz) + 12) * U + 3 * U * p / (1 - p)
                                           + 4 * U * (abs(np.log(p)) + abs(np.log1p(-p))))
    return out, corr, bound


# ---------------------------------------------------------------------------------------------- fused -----
@dataclass(frozen=True)
class FusedCase:
    """rtk_score_packed_bce_f32 against rtk_score_packed_f32 (SIGMOID | SIGMOID_FAST | KERNEL_V3) on the same planes.
    scale: standard deviation of the logits (both saturations occur from ~40 on)."""
    name: str
    B: int
    N: int
    c: int
    eps: float = 0.1
    pad: int = 0
    scale: float = 40.0
    find_eps: bool = False       # search the stored P for a value that some float32 eps maps t0 onto


FUSED_CASES = [
    FusedCase("b1_n1_c4", 1, 1, 4, scale=2.0),
    FusedCase("b31_n127_c31", 31, 127, 31, pad=3),
    FusedCase("b33_n129_c36", 33, 129, 36, eps=0.0),
    FusedCase("b70_n3003_c200", 70, 3003, 200, pad=5),
    FusedCase("b70_n3003_c224_t0_hit", 70, 3003, 224, scale=6.0, find_eps=True),
    FusedCase("b33_n129_c272", 33, 129, 272, pad=1),
    FusedCase("b31_n127_c512", 31, 127, 512),
    FusedCase("b448_n5120_c36_units_over_grid", 448, 5120, 36),
]


def fused_operands(case):
    """v (B, c) and O (N, c): normals with logits of standard deviation case.scale."""
    rng = np.random.default_rng(_seed(case.name))
    v = rng.standard_normal((case.B, case.c)).astype(np.float32)
    O = (rng.standard_normal((case.N, case.c)) * (case.scale / np.sqrt(case.c))).astype(np.float32)
    return v, O


def fused_x_reference(P, t0):
    """What the loss epilogue stores for the probability P it computed, bit for bit."""
    xv = (P - t0).astype(np.float32)
    x = np.where(xv == 0.0, DENORM_MIN, xv)
    x = np.where(P == 0.0, np.float32(-0.0), x)
    return np.where(P == 1.0, np.float32(0.0), x).astype(np.float32)


def find_eps_for(P, N, lo=0.0, hi=1.0):
    """The first stored p below 1 / N (row-major) for which some float32 eps gives float32(eps) / float32(N) == p,
    searched +-6 ulp around p N.  -> (eps, p) or None."""
    Nf = np.float32(N)
    for p in P.reshape(-1):
        if not (0.0 < p < 1.0 / N):
            continue
        e = np.float32(p * Nf)
        cands = [e]
        up = dn = e
        for _ in range(6):
            up, dn = np.nextafter(up, np.float32(2)), np.nextafter(dn, np.float32(-1))
            cands += [up, dn]
        for e in cands:
            if lo < e < hi and e / Nf == p:
                return float(e), p
    return None


def negatives_reference(P, N, eps):
    """float64 sum over the whole block of the BCE terms with every entry taken as a negative, and sum|terms|."""
    t0 = float(constants(N, eps)[0])
    p = P.astype(np.float64)
    lp, lq = L(p), L(1.0 - p)
    return -(t0 * lp + (1.0 - t0) * lq).sum(), (np.abs(t0 * lp) + np.abs((1.0 - t0) * lq)).sum()
