"""Inputs, float64 references, bounds, fp32 emulations and case lists for the softmax cross-entropy loss kernels
(csrc/rtk_ce.hip, csrc/rtk_ce_stream.hip and the skeletons of csrc/rtk_stream_kernel.h), driven through their four C
entry points: no stage 1 and no GEMM enters any bound.

Constants, formed the way the hosts in the .hip files form them: eps32 = float32(eps);
    rtk_ce_rows_f32, rtk_ce_stream_rows_f32 (float64):  t0 = double(eps32) / N, dt = 1 - double(eps32), w = [n_d > 0] dt + eps
    the gradients (fp32):  t0 = eps32 / float32(N), dt = 1.0f - eps32, w = [n_d > 0] dt + eps32, s = g * scale
n_d is the STORED list length pair_ptr[s + 1] - pair_ptr[s] (0 for pair_slot[d] < 0): an out-of-range entry adds no term
but counts in 1 / n_d and in [n_d > 0].  u = 2^-24 is the unit roundoff of fp32.

  CSR      bce_cases.build_csr's lists (ids -1, N and N + 5 in every list of six or more; rows cycling over the lists;
           the last row on slot 0), one row with pair_slot = -1 where the batch has room, and for the matrix-free cases
           entities 0 and N - 1 in every list of two or more (a positive shared by most queries: scatter collisions).
  Z        planted logit rows, one KIND per row (KINDS): normals of sigma 3, 20 and 40, all columns equal, a logit 60
           above the rest at column 0, 255, 256, 2047, 2048 and N - 1, an ascending and a descending ramp, a level of
           +-1000, a row that underflows, -0.0 and a denormal among ordinary values.  ld > N: the padding is NaN.

The exponential.  Every kernel forms exp(a) as exp2(fl(fl(a) * L2E)) with the hardware's exp2 (1 ulp = 2 u) and
L2E = float32(log2 e).  The argument a = z - m (or z - lse, M - m) is a rounded difference of two floats (u |a|), the
constant is off by 0.22 u relative, the product is rounded (u): the exponent moves by at most 2.22 u |a| log2 e, the
result by the relative ARG |a| u with ARG = 2.25.  (The issue's sketch charged log2 e |a| u for the gradient: that
misses the rounding of the product with L2E and the constant's own error; its rows sketch, 2 (m - z) u, has them.)

  rows     ce_rows_kernel: a thread's columns in groups of eight -- fp32 within a group, float64 across groups, one
           rescale S * exp(M - m) per group -- merged at the row maximum in float64.  An element's factor errors
           telescope to ARG (m - z_j) u; weighted by the softmax that is ARG H u with H = sum_j p_j (m - z_j) <= ln N
           (computed per row).  On top: 2 u (exp2), 7 u (the fp32 sum of eight), 2 u per rescale (R = ceil(N / 2048)
           of them), and 2^-50 for the float64 part:
               |lse - ref| <= (ARG H + 9 + 2 R) u,        lse_out adds |lse| u,
               |rows - ref| <= w dlse + 8 u t0 sum|z| + 2^-50 (|w lse| + t0 sum|z| + dt / n_d sum|z_t|)
           (the positives are summed in float64).  exp2 results below 2^-126 may be flushed: N 2^-126, relative to a
           sum >= 1, is inside the 2^-50.
  grad     out = (w exp(z - l) - t0) s, then -fl(fl(dt / n_d) s) on the positives, l = float32(lse_ref) chosen by the
           test and used by the reference, so no lse error enters.  Per element
               |w p s| (6 + ARG |z - l|) u  +  3 u t0 |s|  +  2 u |ref|  +  [positive] 3 u dt / n_d |s|  +  w |s| 2^-126:
           exp2 (2 u), the products with w and s, the subtraction and the positive's two roundings and subtraction;
           the last term is a denormal exponential flushed.
  stream   z = v O^T through the split-fp16 chain (hi + lo with 2^-22 relative per operand, lo x lo dropped: 3 u22 per
           term, u22 = 2^-22; three MFMAs per k-step.  The model of an MFMA: its 16 products of fp16 factors are exact, they
           enter the fp32 accumulator in one fused step, and the accumulator is rounded to nearest once per instruction
           -- one u of the running sum, itself at most the prefix S_j(t) of sum_k |v_k| |O_jk| up to k-step t; fp16
           subnormal lo halves: 2^-39 of the row maxima):
               dz_j = 3 u22 S_j + 3 u sum_t S_j(t) + 2^-39 (max|v| sum|O_j| + max|O_j| sum|v|)   <= kappa u22 S_j,
               kappa = 3 + 0.75 KS,    S_j = sum_k |v_k| |O_jk|.
           Family E has dz = 0 (asserted on the host from the magnitudes).  Forward: the rows bound with sixteen
           columns per lane and tile (15 u), one rescale per tile of a split (R = ceil(tiles / splits)) and the lane
           pair's merge (2 u): (ARG H + 19 + 2 R) u + 1.01 sum_j p_j dz_j; the positives' term is an fp32 chain of
           ceil(n_d / 128) terms per lane and a butterfly: (ceil(n_d / 128) + 10) u dt / n_d sum|z_t| + dt / n_d sum dz_t.
           Backward, per element of dv (gO alike with scale v for O and the query groups for the entity groups):
               sum_j dx_j |O_jk| + 3 u22 sum_j |x_j| |O_jk| + u sum_j r_j |x_j| |O_jk| + floor + the positives,
               dx_j = 1.01 |w p_j| ((3 + ARG |z - l|) u + dz_j) + (w p_j + t0) u + w 2^-126,
           r_j = the fp32 roundings a term passes: three per remaining 16-row group of its split (gO: of the batch) plus
           one per remaining split; floor = 2^-39 (sum_j |O_jk| + max|O| sum_j |x_j|), the fp16 subnormal spacing of
           the lo halves of x (times 2^-14) and of O (scaled to [2^14, 2^15)).

Host-only (numpy).  tests/test_ce_kernel_cases_host.py proves the method without a GPU (fp32 emulations pass, also with
every exponential moved by one ulp; every named mutant fails); tests/test_gpu_ce_kernels.py parametrizes over the same
lists and judges the device's output with the same *_verdict functions.
"""
import math
import zlib
from dataclasses import dataclass

import numpy as np

import bce_cases as bc

U = 2.0 ** -24
U22 = 2.0 ** -22
ARG = 2.25
F0, F1 = np.float32(0), np.float32(1)
L2E32 = np.float32(1.4426950408889634)
CE_NONE = np.float32(-3.0e38)
GRAD_G = -3.0
KINDS = ("n3", "n20", "equal", "dom0", "dom255", "dom256", "dom2047", "dom2048", "domlast", "asc", "desc", "up1000",
         "down1000", "underflow", "zeros", "n40")


def _seed(name):
    return zlib.crc32(name.encode())


def consts32(N, eps):
    """(t0, dt, eps32) as the gradient hosts form them."""
    eps32 = np.float32(eps)
    return eps32 / np.float32(N), F1 - eps32, eps32


def consts64(N, eps):
    """(t0, dt, eps) as the hosts of the rows entries form them, in double from float32(eps)."""
    e = float(np.float32(eps))
    return e / float(N), 1.0 - e, e


def exp32(a, perturb=0):
    """The kernels' exponential in numpy fp32; perturb = +-1 moves every result by one ulp."""
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2((np.asarray(a, dtype=np.float32) * L2E32).astype(np.float32)).astype(np.float32)
    if perturb:
        e = np.nextafter(e, np.float32(np.inf) if perturb > 0 else F0).astype(np.float32)
    return e


# ---------------------------------------------------------------------------------------------- CSR -------
@dataclass(frozen=True)
class Csr:
    slot: np.ndarray        # (B,) int64, -1: no list
    ptr: np.ndarray
    obj: np.ndarray         # out-of-range ids included

    def list_of(self, d):
        s = self.slot[d]
        return self.obj[:0] if s < 0 else self.obj[self.ptr[s]:self.ptr[s + 1]]

    def positives(self, d, N):
        l = self.list_of(d)
        return l[(l >= 0) & (l < N)]

    def stored(self):
        """n_d of every row: the stored list length."""
        return np.array([len(self.list_of(d)) for d in range(len(self.slot))], dtype=np.int64)

    def longest(self):
        return int(np.diff(self.ptr).max())


def _force(seg, pos, val):
    where = np.nonzero(seg == val)[0]
    if len(where):
        seg[where[0]] = seg[pos]
    seg[pos] = val


def build_csr(rng, N, lengths, B, hub=False):
    base = bc.build_csr(rng, N, lengths, B)
    slot, obj = base.slot.copy(), base.obj.copy()
    if B >= len(lengths) + 2:
        slot[B - 2] = -1
    if hub and N >= 4:
        for s in range(len(lengths)):
            seg = obj[base.ptr[s]:base.ptr[s + 1]]
            good = np.nonzero((seg >= 0) & (seg < N))[0]
            if len(good) >= 2:
                _force(seg, good[0], 0)
                _force(seg, good[-1], N - 1)
    return Csr(slot, base.ptr, obj)


def weights(n_d, dt, eps):
    """w_d in the arithmetic of dt and eps (fp32 or float64)."""
    if isinstance(dt, np.float32):
        return (np.where(n_d > 0, dt, F0).astype(np.float32) + eps).astype(np.float32)
    return np.where(n_d > 0, dt, 0.0) + eps


# ---------------------------------------------------------------------------------------------- matrix form
@dataclass(frozen=True)
class RowsCase:
    """rtk_ce_rows_f32 / rtk_ce_grad_f32 on planted logits.  pad: ld - N.  off: floats Z is moved off a 16-byte
    boundary (gradient: the scalar path)."""
    name: str
    N: int
    B: int
    lengths: tuple
    eps: float = 0.1
    pad: int = 0
    off: int = 0

    @property
    def ld(self):
        return self.N + self.pad


ROWS_CASES = [
    RowsCase("n1", 1, 18, (1, 0, 6)),
    RowsCase("n255_eps0", 255, 18, (255, 0, 1), eps=0.0, pad=3),
    RowsCase("n257", 257, 18, (257, 1, 0)),
    RowsCase("n2047_pad", 2047, 18, (256, 0, 600), pad=1),
    RowsCase("n2048_eps0", 2048, 18, (600, 255, 0), eps=0.0, pad=5),
    RowsCase("n2049", 2049, 18, (0, 257, 1)),
    RowsCase("n4097_pad", 4097, 18, (257, 600, 0), pad=7),
    RowsCase("n5889_b70", 5889, 70, (0, 1, 255, 256, 257, 600)),
]

GRAD_CASES = [
    # ld % 4 == 0 and an aligned base: the vector path and its tail, N % 4 = 0, 1, 2, 3
    RowsCase("vec_n4096", 4096, 18, (200, 0, 65)),
    RowsCase("vec_n4097", 4097, 18, (64, 1, 63), pad=3),
    RowsCase("vec_n258", 258, 18, (65, 0, 1), pad=2, eps=0.0),
    RowsCase("vec_n259", 259, 70, (0, 1, 63, 64, 65, 200), pad=1),
    # the scalar path: an odd ld; an aligned ld behind a base moved by 4 bytes
    RowsCase("scalar_odd_ld", 4097, 18, (65, 200, 0)),
    RowsCase("scalar_offset_base", 4096, 18, (63, 64, 0), off=1),
    RowsCase("scalar_n1", 1, 18, (1, 0, 6)),
    # beyond 64 blocks x 4096 columns: every block of the capped grid strides twice
    RowsCase("cap_n270339", 270339, 2, (200, 65), pad=1),
]
CHAINED_CASE = RowsCase("chained_n4097", 4097, 18, (64, 0, 200), pad=3)


def _row(kind, N, rng):
    g = rng.standard_normal(N)
    if kind in ("n3", "n20", "n40"):
        z = float(kind[1:]) * g
    elif kind == "equal":
        z = np.full(N, 1.7)
    elif kind.startswith("dom"):
        z = 3.0 * g
        col = N - 1 if kind == "domlast" else min(int(kind[3:]), N - 1)
        z[col] = np.delete(z, col).max(initial=0.0) + 60.0
    elif kind in ("asc", "desc"):
        z = np.linspace(-30.0, 30.0, N) + 0.01 * g
        z = z[::-1] if kind == "desc" else z
    elif kind in ("up1000", "down1000"):
        z = 3.0 * g + (1000.0 if kind == "up1000" else -1000.0)
    elif kind == "underflow":
        z = -150.0 + g
        few = rng.permutation(N)[:max(1, N // 64)]
        z[few] = 3.0 * g[few]
    else:                                        # "zeros": columns 0, 5 and N - 1 stay ordinary
        z = 3.0 * g
        free = [j for j in rng.permutation(N).tolist() if j not in (0, 5, N - 1)]
        z[free[:N // 8]] = -0.0
        z[free[N // 8:N // 4]] = 1e-40
    return np.ascontiguousarray(z, dtype=np.float64).astype(np.float32)


def plant(case, csr):
    """Z (B, ld) float32, NaN in the padding; row d is of kind KINDS[d % 16]."""
    rng = np.random.default_rng(_seed(case.name) + 1)
    Z = np.full((case.B, case.ld), np.nan, dtype=np.float32)
    for d in range(case.B):
        Z[d, :case.N] = _row(KINDS[d % len(KINDS)], case.N, rng)
    return Z


def setup_rows(case):
    csr = build_csr(np.random.default_rng(_seed(case.name)), case.N, case.lengths, case.B)
    return csr, plant(case, csr)


def lse64(z):
    m = z.max(axis=1)
    return m + np.log(np.exp(z - m[:, None]).sum(axis=1))


def _pos_sums(csr, z, N, mutant=None):
    """Per row: the sum of z over the positives, the sum of |z| over them, the count n_d that divides."""
    B = z.shape[0]
    pz, paz, n = np.zeros(B), np.zeros(B), csr.stored().astype(np.float64)
    for d in range(B):
        l = csr.list_of(d)
        if mutant == "first_256_only":
            l = l[:256]
        t = l % N if mutant == "wrap_ids" and len(l) else l[(l >= 0) & (l < N)]
        pz[d], paz[d] = z[d, t].sum(), np.abs(z[d, t]).sum()
        if mutant == "count_in_range":
            n[d] = len(t)
    return pz, paz, n


def rows_reference(case, Z, csr, mutant=None):
    """float64 (lse, rows) from the fp32 Z.  mutant: a named wrong kernel (host proof)."""
    N = case.N
    t0, dt, eps = consts64(N, case.eps)
    z = Z[:, :N].astype(np.float64)
    zz = z
    if mutant == "drop_last_column":
        zz = z[:, :N - 1] if N > 1 else z
    elif mutant == "duplicate_last_column":
        zz = np.concatenate([z, z[:, N - 1:]], axis=1)
    lse = lse64(zz)
    pz, _, n = _pos_sums(csr, z, N, mutant)
    w = weights(csr.stored(), dt, eps)
    if mutant == "w_one_on_empty":
        w = np.full_like(w, dt + eps)
    t0m = 0.0 if mutant == "no_t0" else t0
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = np.where(csr.stored() > 0, dt / n * pz, 0.0)
    pos = np.where(np.isfinite(pos), pos, 1e30)              # a mutant dividing by zero entries
    return lse, w * lse - t0m * zz.sum(axis=1) - pos


def rows_bounds(case, Z, csr):
    """(bound of lse in float64, of lse_out, of rows_out)."""
    N = case.N
    t0, dt, eps = consts64(N, case.eps)
    z = Z[:, :N].astype(np.float64)
    lse, rows = rows_reference(case, Z, csr)
    m = z.max(axis=1)
    p = np.exp(z - lse[:, None])
    H = (p * (m[:, None] - z)).sum(axis=1)
    R = -(-N // 2048)
    dl = (ARG * H + 9 + 2 * R) * U + 2.0 ** -50 * (1.0 + np.abs(lse))
    w = weights(csr.stored(), dt, eps)
    _, paz, n = _pos_sums(csr, z, N)
    az = np.abs(z).sum(axis=1)
    posmag = np.where(n > 0, dt / np.maximum(n, 1) * paz, 0.0)
    db = w * dl + 8 * U * t0 * az + 2.0 ** -50 * (np.abs(w * lse) + t0 * az + posmag)
    return dl, dl + np.abs(lse) * U, db


def emul_rows(case, Z, csr, perturb=0, rescale=True):
    """ce_rows_kernel in numpy: fp32 within a group of eight, float64 across -> (lse_out float32, rows float64)."""
    N, B = case.N, case.B
    t0, dt, eps = consts64(N, case.eps)
    C = -(-N // 2048)
    Zp = np.full((B, C * 2048), CE_NONE, dtype=np.float32)
    Zp[:, :N] = Z[:, :N]
    ok = np.zeros((B, C * 2048), dtype=bool)
    ok[:, :N] = True
    Zp, ok = Zp.reshape(B, C, 8, 256), ok.reshape(B, C, 8, 256)
    M = np.full((B, 256), CE_NONE, dtype=np.float32)
    S, SZ = np.zeros((B, 256)), np.zeros((B, 256))
    for ch in range(C):
        m, zs = M.copy(), np.zeros((B, 256), dtype=np.float32)
        for u in range(8):
            zs = (zs + np.where(ok[:, ch, u], Zp[:, ch, u], F0)).astype(np.float32)
            m = np.maximum(m, Zp[:, ch, u])
        ts = np.zeros((B, 256), dtype=np.float32)
        for u in range(8):
            ts = (ts + np.where(ok[:, ch, u], exp32(Zp[:, ch, u] - m, perturb), F0)).astype(np.float32)
        S = S * (exp32(M - m, perturb).astype(np.float64) if rescale else 1.0) + ts.astype(np.float64)
        M = m
        SZ += zs.astype(np.float64)
    m = M.max(axis=1)
    with np.errstate(under="ignore"):
        a = np.where(S > 0, S * np.exp(M.astype(np.float64) - m[:, None].astype(np.float64)), 0.0)
    lse = m.astype(np.float64) + np.log(a.sum(axis=1))
    pz, _, n = _pos_sums(csr, Z[:, :N].astype(np.float64), N)
    w = weights(csr.stored(), dt, eps)
    rows = w * lse - t0 * SZ.sum(axis=1) - np.where(n > 0, dt / np.maximum(n, 1) * pz, 0.0)
    return lse.astype(np.float32), rows


def _ratio(err, bound):
    """Largest error / bound; an exact result against a bound of zero counts as 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0.0, 0.0, err / bound).max())


def rows_verdict(case, Z, csr, got_lse, got_rows):
    """-> (largest error / bound of lse_out, of rows_out).  Both are <= 1 for a right kernel."""
    lse, rows = rows_reference(case, Z, csr)
    _, bl, br = rows_bounds(case, Z, csr)
    if not (np.isfinite(got_lse).all() and np.isfinite(got_rows).all()):
        return np.inf, np.inf
    return _ratio(np.abs(got_lse.astype(np.float64) - lse), bl), _ratio(np.abs(got_rows - rows), br)


def grad_scale(case):
    return np.float32(1.0 / case.B)


def grad_reference(case, Z, csr, lse32, mutant=None):
    """float64 (B, N): (w exp(z - l) - t0) s - [positive] dt / n_d s, from the fp32 constants and the float l."""
    N, B = case.N, case.B
    t0, dt, eps = consts32(N, case.eps)
    s = float(np.float32(GRAD_G) * grad_scale(case))
    n = csr.stored()
    w = weights(n, dt, eps).astype(np.float64)
    l = lse32.astype(np.float64)
    if mutant == "neighbour_w":
        w = np.roll(w, 1)
    if mutant == "neighbour_lse":
        l = np.roll(l, 1)
    z = Z[:, :N].astype(np.float64)
    with np.errstate(over="ignore"):
        out = (w[:, None] * np.exp(z - l[:, None]) - (0.0 if mutant == "no_t0" else float(t0))) * s
    users = np.bincount(csr.slot[csr.slot >= 0], minlength=len(csr.ptr) - 1)
    for d in range(B):
        l_d = csr.list_of(d)
        if mutant == "first_64_only":
            l_d = l_d[:64]
        t = l_d[(l_d >= 0) & (l_d < N)]
        if len(t):
            times = users[csr.slot[d]] if mutant == "once_per_slot_user" else 1
            out[d, t] -= times * float(dt) / float(n[d]) * s
    return out


def grad_bound(case, Z, csr, lse32, ref):
    N = case.N
    t0, dt, eps = consts32(N, case.eps)
    s = abs(float(np.float32(GRAD_G) * grad_scale(case)))
    n = csr.stored()
    w = weights(n, dt, eps).astype(np.float64)
    a = Z[:, :N].astype(np.float64) - lse32.astype(np.float64)[:, None]
    with np.errstate(over="ignore"):
        wps = w[:, None] * np.exp(a) * s
    b = wps * (6 + ARG * np.abs(a)) * U + 3 * U * float(t0) * s + 2 * U * np.abs(ref) + (w * s * 2.0 ** -126)[:, None]
    for d in range(case.B):
        t = csr.positives(d, N)
        if len(t):
            b[d, t] += 3 * U * float(dt) / float(n[d]) * s
    return b


def emul_grad(case, Z, csr, lse32, perturb=0):
    """The two passes of rtk_ce_grad_f32 in numpy fp32, on a copy of the whole (B, ld) block."""
    N = case.N
    t0, dt, eps = consts32(N, case.eps)
    s = np.float32(GRAD_G) * grad_scale(case)
    n = csr.stored()
    w = weights(n, dt, eps)
    out = Z.copy()
    e = exp32(Z[:, :N] - lse32[:, None], perturb)
    out[:, :N] = ((w[:, None] * e).astype(np.float32) - t0) * s
    for d in range(case.B):
        t = csr.positives(d, N)
        if len(t):
            out[d, t] -= dt / np.float32(n[d]) * s
    return out


def grad_verdict(case, Z, csr, lse32, got_full):
    """got_full: the (B, ld) block afterwards -> largest error / bound; inf when the padding changed its bits."""
    N = case.N
    if not np.array_equal(got_full[:, N:].view(np.uint32), Z[:, N:].view(np.uint32)):
        return np.inf
    ref = grad_reference(case, Z, csr, lse32)
    b = grad_bound(case, Z, csr, lse32, ref)
    got = got_full[:, :N].astype(np.float64)
    if not np.isfinite(got).all():
        return np.inf
    return _ratio(np.abs(got - ref), b)


# ---------------------------------------------------------------------------------------------- matrix-free
STREAM_LENGTHS = (0, 1, 31, 32, 33, 127, 128, 129, 300)


@dataclass(frozen=True)
class StreamCase:
    """rtk_ce_stream_rows_f32 / rtk_ce_stream_grad_f32 on planes packed from v.  family E: exact logits; G: normals
    with std(z) ~ sigma."""
    family: str
    B: int
    N: int
    c: int
    eps: float = 0.1
    sigma: float = 3.0
    lengths: tuple = STREAM_LENGTHS

    @property
    def name(self):
        return f"{self.family.lower()}_b{self.B}_n{self.N}_c{self.c}" + ("_eps0" if self.eps == 0.0 else "") + \
            (f"_s{int(self.sigma)}" if self.sigma != 3.0 else "")

    @property
    def ks(self):
        return (self.c + 15) // 16


_SHAPES = [(1, 1, 4), (31, 33, 16), (33, 95, 20), (32, 3003, 36), (129, 3003, 64), (513, 257, 32), (70, 4099, 100),
           (70, 3003, 208)]
KS_CASES = [StreamCase("E", 33, 97, 16 * ks) for ks in range(1, 14)]
SHAPE_CASES = [StreamCase(f, B, N, c, eps=0.0 if (f, c) in (("E", 20), ("G", 36)) else 0.1,
                          lengths=(1,) if B == 1 else STREAM_LENGTHS) for (B, N, c) in _SHAPES for f in ("E", "G")]
STREAM_CASES = KS_CASES + SHAPE_CASES + [StreamCase("G", 31, 33, 4, sigma=25.0)]
SINGLE_OUTPUT_CASES = [c for c in SHAPE_CASES if c.c in (36, 208)]


def splits_of(B):
    return max(1, 256 // max(1, (-(-B // 32) + 3) // 4))


def split_edges(B, N):
    S, n_t = splits_of(B), -(-N // 32)
    return [(n_t * sp) // S for sp in range(S + 1)]


def pack_shift(mx):
    mx = float(mx)
    if not (mx > 0.0 and math.isfinite(mx)):
        return 0
    return int(np.clip(14 - (math.frexp(mx)[1] - 1), -100, 100))


@dataclass(frozen=True)
class StreamData:
    csr: Csr
    v: np.ndarray           # (B, c) float32
    O: np.ndarray           # (N, c) float32
    z: np.ndarray           # (B, N) float64: the product of the fp32 operands


def stream_operands(case):
    rng = np.random.default_rng(_seed(case.name))
    B, N, c = case.B, case.N, case.c
    csr = build_csr(rng, N, case.lengths, B, hub=True)
    if case.family == "E":
        need = 2.5 ** 2 / (2.0 * c)                           # E[v^2] for std(z) = 2.5 with E[O^2] = 2
        e = math.ceil(0.5 * math.log2(need / (0.9 * 2.0 ** -6)))
        r = need / 4.0 ** e / 0.9
        p = (r - 2.0 ** -8) / (2.0 ** -6 - 2.0 ** -8)
        mag = np.where(rng.random((B, c)) < p, 2.0 ** -3, 2.0 ** -4) * np.where(rng.random((B, c)) < 0.1, 0.0, 1.0)
        v = (mag * rng.choice([-1.0, 1.0], size=(B, c)) * 2.0 ** e).astype(np.float32)
        O = rng.integers(-2, 3, size=(N, c)).astype(np.float32)
        O[N - 1] = np.where(v[0] < 0, -2.0, 2.0)              # the last valid row: query 0's largest possible logit
    else:
        v = rng.standard_normal((B, c)).astype(np.float32)
        O = (rng.standard_normal((N, c)) * (case.sigma / math.sqrt(c))).astype(np.float32)
        k = 4.5 * case.sigma / float(v[0].astype(np.float64) @ v[0].astype(np.float64))
        for _ in range(40):
            O[N - 1] = (v[0] * k).astype(np.float32)
            z0 = O.astype(np.float64) @ v[0].astype(np.float64)
            if N == 1 or z0[N - 1] > np.delete(z0, N - 1).max() + 1.0:
                break
            k *= 1.2
    return StreamData(csr, v, O, v.astype(np.float64) @ O.astype(np.float64).T)


def chain_bound(case, data):
    """dz (B, N): the logit error of the three-product hi/lo chain (zeros for family E)."""
    B, N = case.B, case.N
    if case.family == "E":
        return np.zeros((B, N))
    av, aO = np.abs(data.v.astype(np.float64)), np.abs(data.O.astype(np.float64))
    full = av @ aO.T
    pre = np.zeros((B, N))
    for t in range(case.ks):
        k1 = min(16 * (t + 1), case.c)
        pre += av[:, :k1] @ aO[:, :k1].T
    floor = 2.0 ** -39 * (av.max(axis=1)[:, None] * aO.sum(axis=1)[None, :] + aO.max(axis=1)[None, :] * av.sum(axis=1)[:, None])
    return 3 * U22 * full + 3 * U * 1.001 * pre + floor


def _pos_dense(case, csr, coef, stray=False):
    """(B, N) float64: coef[d] on the in-range positives of row d.  stray: the pair_slot = -1 row scatters the first
    list of two or more entries (a mutant)."""
    Y = np.zeros((case.B, case.N))
    for d in range(case.B):
        Y[d, csr.positives(d, case.N)] = coef[d]
        if stray and csr.slot[d] < 0:
            s = int(np.argmax(np.diff(csr.ptr) >= 2))
            l = csr.obj[csr.ptr[s]:csr.ptr[s + 1]]
            Y[d, l[(l >= 0) & (l < case.N)]] = 0.9 / len(l)
    return Y


def stream_forward(case, data, mutant=None):
    """float64 (lse, rows) and their bounds (lse, lse_out, rows)."""
    B, N = case.B, case.N
    t0, dt, eps = consts64(N, case.eps)
    z, csr = data.z, data.csr
    n = csr.stored()
    w = weights(n, dt, eps)
    lse = lse64(z)
    edges = split_edges(B, N)
    if mutant == "merge_without_split_maximum":
        m, s = z.max(axis=1), np.zeros(B)
        for a, b in zip(edges[:-1], edges[1:]):
            if b > a:
                zz = z[:, 32 * a:min(32 * b, N)]
                s += np.exp(zz - zz.max(axis=1)[:, None]).sum(axis=1)
        lse = m + np.log(s)
    pz, paz, _ = _pos_sums(csr, z, N)
    coef = np.where(n > 0, dt / np.maximum(n, 1), 0.0)
    rows = w * lse - t0 * z.sum(axis=1) - coef * pz
    dz = chain_bound(case, data)
    m = z.max(axis=1)
    p = np.exp(z - lse64(z)[:, None])
    H = (p * (m[:, None] - z)).sum(axis=1)
    R = max(b - a for a, b in zip(edges[:-1], edges[1:]))
    dl = (ARG * H + 19 + 2 * R) * U + 1.01 * (p * dz).sum(axis=1) + 2.0 ** -50 * (1.0 + np.abs(lse))
    az = np.abs(z).sum(axis=1)
    pdz = np.array([dz[d, csr.positives(d, N)].sum() for d in range(B)])
    db = w * dl + t0 * (16 * U * az + dz.sum(axis=1)) + coef * ((-(-n // 128) + 10) * U * paz + pdz) \
        + 2.0 ** -50 * (np.abs(w * lse) + t0 * az + coef * paz)
    return lse, rows, dl, dl + np.abs(lse) * U, db


def stream_scale(case):
    return np.float32(GRAD_G) * np.float32(1.0 / case.B)      # the device scalar scale[0] = g / batch


def _term_roundings(case):
    """r_j for dv (per entity) and r_d for gO (per query): the fp32 roundings a term of the tile product passes."""
    B, N = case.B, case.N
    edges = np.asarray(split_edges(B, N))
    tile = np.arange(N) // 32
    sp = np.searchsorted(edges, tile, side="right") - 1
    nonempty = np.diff(edges) > 0
    after = np.cumsum(nonempty[::-1])[::-1]                   # non-empty splits from sp on
    groups_left = 2 * (edges[sp + 1] - tile) - (np.arange(N) % 32) // 16
    r_j = 3 * groups_left + after[sp] + 2
    n_g = 2 * -(-B // 32)
    r_d = 3 * (n_g - np.arange(B) // 16) + 2
    return r_j.astype(np.float64), r_d.astype(np.float64)


def stream_backward(case, data, lse32, mutant=None):
    """float64 dv (B, c), gO (N, c), their bounds and the floors inside the bounds."""
    B, N, c = case.B, case.N, case.c
    t0, dt, eps = [x for x in consts32(N, case.eps)]
    z, csr = data.z, data.csr
    n = csr.stored()
    w = weights(n, dt, eps).astype(np.float64)
    s = float(stream_scale(case))
    O64, v64 = data.O.astype(np.float64), data.v.astype(np.float64)
    sv = s * v64
    a = z - lse32.astype(np.float64)[:, None]
    wp = w[:, None] * np.exp(a)
    x = wp - float(t0)
    coef = np.where(n > 0, float(dt) / np.maximum(n, 1), 0.0)
    Y = _pos_dense(case, csr, coef)
    Yg = _pos_dense(case, csr, coef, stray=True) if mutant == "scatter_slot_minus_one" else Y
    Od, svd, xm = O64, sv, x
    if mutant == "x_lo_dropped":
        xm = (x * 16384.0).astype(np.float16).astype(np.float64) / 16384.0
    if mutant == "O_lo_dropped":
        up = 2.0 ** pack_shift(np.abs(data.O).max())
        Od = (O64 * up).astype(np.float16).astype(np.float64) / up
    if mutant == "sv_lo_dropped":
        up = 2.0 ** pack_shift(np.abs(sv).max())
        svd = (sv * up).astype(np.float16).astype(np.float64) / up
    dv = xm @ Od - Y @ O64
    gO = xm.T @ svd - Yg.T @ sv
    if mutant == "column_past_N":
        dv = dv + np.outer(x[:, N - 1], O64[N - 1])
    if mutant == "query_past_B":
        gO = gO + np.outer(x[B - 1], sv[B - 1])
    # bounds
    dz = chain_bound(case, data)
    dx = 1.01 * wp * ((3 + ARG * np.abs(a)) * U + dz) + (wp + float(t0)) * U + (w * 2.0 ** -126)[:, None]
    ax, aO, asv = np.abs(x), np.abs(O64), np.abs(sv)
    r_j, r_d = _term_roundings(case)
    P = (Y > 0).astype(np.float64)
    chain = (32 * -(-n // 128) + 6).astype(np.float64)
    dv_floor = 2.0 ** -39 * (aO.sum(axis=0)[None, :] + aO.max() * ax.sum(axis=1)[:, None])
    dv_sweep = dx @ aO + 3 * U22 * (ax @ aO) + U * ((ax * r_j[None, :]) @ aO)
    dv_b = dv_sweep + dv_floor + (chain * U * coef)[:, None] * (P @ aO) + 2 * U * np.abs(dv)
    m_j = P.sum(axis=0)
    gO_floor = 2.0 ** -39 * (asv.sum(axis=0)[None, :] + asv.max() * ax.sum(axis=0)[:, None])
    gO_sweep = dx.T @ asv + (3 * U22 + U) * (ax.T @ asv) + U * ((ax * r_d[:, None]).T @ asv)
    gO_b = gO_sweep + gO_floor + ((m_j + 6) * U)[:, None] * ((P * coef[:, None]).T @ asv) + 2 * U * np.abs(gO)
    return dict(dv=dv, gO=gO, dv_b=dv_b, gO_b=gO_b, dv_floor=dv_floor, gO_floor=gO_floor, x=x, w=w,
                dv_sweep=dv_sweep, gO_sweep=gO_sweep, dv_mass=ax @ aO, gO_mass=ax.T @ asv)


def _split16(y):
    hi = y.astype(np.float16)
    return hi.astype(np.float32), (y - hi.astype(np.float32)).astype(np.float16).astype(np.float32)


def emul_stream_grad(case, data, lse32, perturb=0):
    """The link of the backward in numpy fp32: x from the fp32 logit, the 2^14 hi/lo split, three fp32 products
    against the hi/lo split of O (dv) and of scale v (gO), the positives on top."""
    N = case.N
    t0, dt, eps = consts32(N, case.eps)
    csr = data.csr
    n = csr.stored()
    w = weights(n, dt, eps)
    z32 = data.z.astype(np.float32)
    x = ((w[:, None] * exp32(z32 - lse32[:, None], perturb)).astype(np.float32) - t0).astype(np.float32)
    xh, xl = _split16(x * np.float32(16384.0))
    coef = np.where(n > 0, dt / np.maximum(n, 1).astype(np.float32), F0).astype(np.float32)
    Y = _pos_dense(case, csr, coef.astype(np.float64)).astype(np.float32)

    def product(A_h, A_l, T):
        sh = pack_shift(np.abs(T).max())
        th, tl = _split16((T * np.float32(2.0 ** sh)).astype(np.float32))
        acc = (A_h @ th + A_h @ tl + A_l @ th).astype(np.float32)
        return (acc * np.float32(2.0 ** (-14 - sh))).astype(np.float32)

    sv = (data.v * stream_scale(case)).astype(np.float32)
    dv = product(xh, xl, data.O) - (Y @ data.O).astype(np.float32)
    gO = product(xh.T.copy(), xl.T.copy(), sv) - (Y.T @ sv).astype(np.float32)
    return dv, gO


def stream_backward_verdict(ref, got_dv, got_gO):
    """-> (largest error / bound of dv, of gO); inf when a row of mass w_d = 0 has a non-zero bit in dv."""
    if not (np.isfinite(got_dv).all() and np.isfinite(got_gO).all()):
        return np.inf, np.inf
    r_dv = _ratio(np.abs(got_dv.astype(np.float64) - ref["dv"]), ref["dv_b"])
    if np.any(np.ascontiguousarray(got_dv, dtype=np.float32)[ref["w"] == 0.0].view(np.uint32) != 0):
        r_dv = np.inf
    return r_dv, _ratio(np.abs(got_gO.astype(np.float64) - ref["gO"]), ref["gO_b"])


def stream_forward_verdict(ref, got_lse, got_rows):
    """ref: stream_forward's tuple -> (largest error / bound of lse_out, of loss_rows_out)."""
    lse, rows, _, bl, br = ref
    if not (np.isfinite(got_lse).all() and np.isfinite(got_rows).all()):
        return np.inf, np.inf
    return _ratio(np.abs(got_lse.astype(np.float64) - lse), bl), _ratio(np.abs(got_rows - rows), br)
