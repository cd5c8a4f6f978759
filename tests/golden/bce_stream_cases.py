"""Inputs, float64 references, bounds, fp32 emulations, mutants and case lists for the matrix-free BCE loss kernels
(csrc/rtk_bce_stream.hip on the skeletons of csrc/rtk_stream_kernel.h), driven through their four C entry points
rtk_bce_stream_rows_f32, rtk_bce_stream_grad_o_f32 and the two *_part_f32 forms on planes packed from a given v
(rtk_pack_query_vectors): no stage 1 and no GEMM enters any bound.  The method is ce_kernel_cases.py's; what is shared
with it (the chain bound dz, the roundings per term r_j / r_d, the fp16 split, the CSR builder) is imported from there.

Constants, formed the way the host in the .hip file forms them (fp32):
    eps32 = float32(eps),  t0 = eps32 / float32(n_ent),  dt = 1.0f - eps32,  scale = g / (B N) with g = -3 (one case: 1.0).
n_ent is the GLOBAL entity count, in the block form too.  u = 2^-24, u22 = 2^-22.

Operands
  E, G     ce_kernel_cases.stream_operands' two families (E: one significant bit per operand, logits exact in fp32,
           dz = 0; G: normals, dz = chain_bound) with two changes, because a logistic follows: the dominant last row of
           the softmax cases is replaced by an ordinary row, and an entity row whose largest |z| over the batch exceeds
           14.5 is shrunk (G: scaled; E: halved towards zero, still integers), so that |z| + dz <= 15 (asserted).
  S        saturating: v and O hold multiples of 0.5 with at most 9 significant bits, every logit is exact in fp32 and
           lies on a lattice of step 0.5.  Query d is of kind d % 5: ordinary, p == 1.0f planted (z >= 22) at columns
           0, 31, 32 and N - 1, p == 0.0f planted (z <= -112) at the same columns, p == 1.0f again from another level,
           and a row on which EVERY column saturates (z = +-150 + ...).  Columns 5 and N - 2 saturate for every query
           (rows of gO that no term touches).  31 and 32 are forced into every list of 33 or more, 0 and N - 1 are the
           hubs, so each planted level falls on listed positives and on negatives (asserted on the host).
  CSR      ce_kernel_cases.build_csr with hubs: entities 0 and N - 1 in every list of two or more, the ids -1, N and
           N + 5 in every list of six or more, one pair_slot = -1 row, the last row on slot 0 (the empty list), list
           lengths 0, 1, 31, 32, 33, 127, 128, 129, 300.  No object occurs twice in a list: that is the precondition of
           include/rtucker_hip.h ("every object of a pair once"), the kernels do not deduplicate.

No ambiguous element.  A saturated element moves x by about 1, so no logit may lie where saturation hangs on the last
ulp of an exponential: 1 + e rounds to 1 from z = ln 2^24 = 16.6355 on, in both logistics; for z in [-89.5, -86.5] the
exact logistic returns subnormals or 0 (expf overflows at 88.72) and v_rcp_f32 flushes.  assert_unambiguous checks for
every case, from the float64 logit +- dz, that none is within 0.1 of 16.6355 or inside [-89.5, -86.5]; |z| + dz <= 15
for E and G and S's lattice (nothing in (8.5, 21.5) or (-111.5, -8.5)) make that hold by construction.  The reference's
rule is then the kernel's: p == 1.0f iff z > 16.6355, p == 0.0f iff z < -88.

References (float64, from z = v O^T of the fp32 operands; p = split_cases.sigmoid64(z), ln p = -ln(1 + e^-z) and
ln(1 - p) = -ln(1 + e^z) formed directly):
    rows[d] = -sum_j [y ln p + (1 - y) ln(1 - p)],  y = dt [j in P_d] + t0; a saturated element has the logs
              (0, -100) or (-100, 0): the clamp acts there and nowhere else
    x[d, j] = p - t0, 0 where saturated;  the positives add -dt, 0 where saturated
    dv = X O,  gO = X^T (scale v)       (X with the positives' share)

Bounds, per element.  Let dz be the logit's chain error and, for an element that is not saturated,
    darg = (ARG |z| + 2) u              fast:  s = srow kcol carries fl(-log2 e) (0.22 u), the product acc s is rounded
                                        (u), both times |z|; v_exp_f32 at 1 ulp (2 u)
           (ARG |z| + 2 EXPF_ULP) u     exact: the product rounded, ocml expf at EXPF_ULP ulp
    dp   = 1.01 p (1 - p) (darg + dz) + k u p,   k = 3 (1 + e rounded, v_rcp_f32 at 1 ulp) or 2 (1 + e, IEEE divide):
the error of e enters p = 1 / (1 + e) with the weight e / (1 + e)^2 = p (1 - p), but the roundings of 1 + e and of the
reciprocal are ABSOLUTE errors k u p of a number near 1.  The kernel forms ln(1 - p) from that fp32 p, so its error is
-ln(1 - (dp + u (1 - p)) / (1 - p)): relative to 1 - p, not to p.  At z = 15, 1 - p = 3.1e-7 while dp = 1.8e-7.  This
is the conditioning of BCE on fp32 probabilities, and it is in the bound, not in a tolerance (the bound asserts
(dp + u (1 - p)) / (1 - p) < 1, which |z| <= 15 guarantees).  Saturated elements have dp = 0: their p is exact.
  rows     per element: t0 (Lp + 4 u |ln p|) + (1 - t0) (Lq + 4 u |ln(1 - p)|) with Lp = -ln(1 - dp / p), Lq as above and
           rtk_clog's own error 4 u |ln| (v_log_f32 at 1 ulp = 2 u, the product with fl(ln 2) and that constant; 0 on a
           saturated element, whose logs are exact), the products with t0 (u) and with fl(1 - t0) (2 u), the add (u) and
           the sixteen fp32 adds per lane and tile (16 u 1.01 of the group's |terms|, summed over the row: of the row's);
           float64 from there: 2^-50 of the sum of |terms|.  A positive: dt (Lp + Lq + 4 u (|ln p| + |ln(1 - p)|)) +
           2 u dt |ln p - ln(1 - p)| (the difference, the product), and the lane's fp32 chain of ceil(n_d / 128) terms
           with the butterfly: (ceil(n_d / 128) + 10) u dt sum_t |ln p - ln(1 - p)| (n_d the stored list length).
  dv, gO   ce_kernel_cases.stream_backward's terms with the BCE dx = dp + u |x| (0 where saturated) in place of the
           softmax's: sum_j dx_j |O_jk| + 3 u22 sum_j |x_j| |O_jk| (the split of x, of O, lo x lo dropped)
           + u sum_j r_j |x_j| |O_jk| (the fp32 roundings a term passes) + the fp16-subnormal floor
           2^-39 (sum_j |O_jk| + max|O| sum_j |x_j|) + the positives' chain (32 ceil(n_d / 128) + 6) u dt sum_t |O_tk|
           + 2 u |dv|; gO alike with scale v for O (one more u: scale * v is rounded), r_d for r_j and (m_j + 6) u for
           the chain of the m_j positives the ordered scatter adds into row j.
  blocks   rows and dv shares summed (dv in fp32, block order), gO concatenated, against the WHOLE-matrix reference at
           TWICE the whole-matrix bound, for the reason ce_part_cases.py gives: the fp32 sums run in another order
           (per block, then over blocks) and the power of two of O in the dv product is the block's own.
A query whose every column and every positive is saturated has a dv row of zero bits, an entity that no unsaturated
element touches has a gO row of +0.0: verdict returns inf otherwise.

Mutants (MUTANTS): a reference that is wrong in one named way, see reference().  tests/test_bce_stream_cases_host.py
shows on the host that the fp32 emulation (emul, every exponential movable by one ulp) is inside every bound on every
case and that every mutant is outside on at least one; tests/test_gpu_bce_stream_kernels.py judges the device with the
same verdict.  Host-only (numpy).
"""
import math
import zlib
from dataclasses import dataclass

import numpy as np

import bce_cases as bc
import ce_kernel_cases as cc
import split_cases as sc

U, U22, ARG = cc.U, cc.U22, cc.ARG
F0, F1 = cc.F0, cc.F1
GRAD_G = cc.GRAD_G
SAT_HI = math.log(2.0 ** 24)                  # 16.6355: from here on 1 + e rounds to 1
SUB_LO, SUB_HI = -89.5, -86.5                 # subnormal or flushed probabilities
Z_MAX = 15.0                                  # families E and G
NL2E32 = np.float32(-1.4426950408889634)
LN2_32 = np.float32(0.6931471805599453)
MODES = ("exact", "fast")
MUTANTS = ("saturated_x_kept", "saturated_positive_kept", "positive_without_negative_term", "no_t0_in_x",
           "local_smoothing", "positive_in_other_block_counted", "column_past_N", "query_past_B", "x_lo_dropped",
           "O_lo_dropped", "sv_lo_dropped", "scatter_slot_minus_one", "log_not_clamped", "first_128_positives_only")
BLOCK_MUTANTS = ("local_smoothing", "positive_in_other_block_counted")


def _seed(name):
    return zlib.crc32(name.encode())


# ---------------------------------------------------------------------------------------------- cases -----
@dataclass(frozen=True)
class Case:
    """family E, G (std(z) ~ sigma) or S.  unit_scale: scale[0] = 1.0 instead of g / (B N).  below: every known object
    lies below this entity (0: anywhere)."""
    family: str
    B: int
    N: int
    c: int
    eps: float = 0.1
    sigma: float = 3.0
    lengths: tuple = cc.STREAM_LENGTHS
    unit_scale: bool = False
    below: int = 0

    @property
    def name(self):
        return f"{self.family.lower()}_b{self.B}_n{self.N}_c{self.c}" + ("_eps0" if self.eps == 0.0 else "") + \
            (f"_eps{self.eps}" if self.eps not in (0.0, 0.1) else "") + \
            (f"_s{int(self.sigma)}" if self.sigma != 3.0 else "") + ("_scale1" if self.unit_scale else "") + (f"_below{self.below}" if self.below else "")

    @property
    def ks(self):
        return (self.c + 15) // 16


KS_CASES = [Case("E", 33, 97, 16 * ks) for ks in range(1, 14)]
SHAPE_CASES = [Case(f, B, N, c, eps=0.0 if (f, c) in (("E", 20), ("G", 36)) else 0.1,
                    lengths=(1,) if B == 1 else cc.STREAM_LENGTHS) for (B, N, c) in cc._SHAPES for f in ("E", "G")]
SIGMA6_CASE = Case("G", 33, 95, 20, sigma=6.0)
UNIT_SCALE_CASE = Case("G", 31, 33, 16, unit_scale=True)
S_CASES = [Case("S", 33, 97, 16), Case("S", 70, 3003, 36), Case("S", 70, 3003, 208)]
CASES = KS_CASES + SHAPE_CASES + [SIGMA6_CASE, UNIT_SCALE_CASE] + S_CASES


@dataclass(frozen=True)
class PartCase:
    """A Case and the cuts of [0, N) into blocks."""
    case: Case
    cuts: tuple

    @property
    def name(self):
        return self.case.name + "_cuts" + "_".join(str(x) for x in self.cuts[1:-1])

    @property
    def blocks(self):
        return [(a, b - a) for a, b in zip(self.cuts[:-1], self.cuts[1:])]


def _parts(c):
    base, below = Case("G", 70, 3003, c), Case("G", 70, 3003, c, below=2000)
    return [PartCase(base, (0, 1501, 3003)),                                     # the cut is inside a tile
            PartCase(base, (0, 1000, 1001, 3003)),                               # a block of one row
            PartCase(below, (0, 2000, 3003)),                                    # a block without positives
            PartCase(base, tuple(3003 * i // 8 for i in range(9)))]              # eight near-equal blocks


PART_CASES = _parts(36) + _parts(208) + [PartCase(S_CASES[1], (0, 1501, 3003))]
WHOLE_BLOCK_CASES = [S_CASES[1], next(k for k in SHAPE_CASES if (k.family, k.c) == ("G", 208))]
MUTANT_PART = PartCase(Case("G", 33, 64, 20, eps=0.5), (0, 32, 64))              # n_ent 64 in two blocks of 32
MUTANT_CASES = [S_CASES[0], S_CASES[1], SIGMA6_CASE, UNIT_SCALE_CASE] + \
    [k for k in SHAPE_CASES if (k.B, k.N) in ((33, 95), (32, 3003), (129, 3003))]


# ---------------------------------------------------------------------------------------------- operands --
def plant_columns(N):
    return sorted({0, 31, 32, N - 1})


def dead_columns(N):
    return [5, N - 2]


def _saturating(case):
    rng = np.random.default_rng(_seed(case.name))
    B, N, c = case.B, case.N, case.c
    assert N >= 97 and c >= 16
    base = cc.build_csr(rng, N, case.lengths, B, hub=True)
    obj = base.obj.copy()
    for s in range(len(case.lengths)):
        seg = obj[base.ptr[s]:base.ptr[s + 1]]
        good = np.nonzero((seg >= 0) & (seg < N))[0]
        if len(good) >= 33:
            cc._force(seg, good[1], 31)
            cc._force(seg, good[2], 32)
            cc._force(seg, good[3], 5)                     # a listed positive on a column that saturates for every query
    v, O = np.zeros((B, c), dtype=np.float32), np.zeros((N, c), dtype=np.float32)
    kind = np.arange(B) % 5
    v[:, 0] = np.array([0.0, 1.0, -2.0, 0.5, 0.0])[kind]
    v[kind == 4, 1] = 150.0
    v[:, 2] = 1.0
    O[plant_columns(N), 0] = 60.0
    O[:, 1] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    O[dead_columns(N), 2] = 200.0
    for d in range(B):
        v[d, rng.permutation(np.arange(3, c))[:4]] = rng.choice([-1.0, -0.5, 0.5, 1.0], size=4)
    O[:, 3:] = rng.integers(-2, 3, size=(N, c - 3))
    return cc.Csr(base.slot, base.ptr, obj), v, O


def _z(v, O):
    return v.astype(np.float64) @ O.astype(np.float64).T


def operands(case):
    """-> ce_kernel_cases.StreamData(csr, v, O, z)."""
    B, N, c = case.B, case.N, case.c
    if case.family == "S":
        csr, v, O = _saturating(case)
    else:
        base = cc.stream_operands(cc.StreamCase(case.family, B, N, c, eps=case.eps, sigma=case.sigma, lengths=case.lengths))
        csr, v, O = base.csr, base.v, base.O.copy()
        rng = np.random.default_rng(_seed(case.name) + 7)
        if case.family == "E":
            O[N - 1] = rng.integers(-2, 3, size=c)
            for _ in range(3):
                over = np.abs(_z(v, O)).max(axis=0) > 14.5
                O[over] = np.trunc(O[over] / 2.0)
        else:
            O[N - 1] = rng.standard_normal(c) * (case.sigma / math.sqrt(c))
            f = np.minimum(1.0, 14.5 / np.maximum(np.abs(_z(v, O)).max(axis=0), 1e-30))
            O = (O.astype(np.float64) * f[:, None]).astype(np.float32)
    if case.below:
        rng = np.random.default_rng(_seed(case.name) + 11)
        low = cc.build_csr(rng, case.below, case.lengths, B, hub=True)
        obj = low.obj.copy()
        obj[low.obj == case.below] = N                       # the out-of-range ids of the smaller range
        obj[low.obj == case.below + 5] = N + 5
        csr = cc.Csr(low.slot, low.ptr, obj)
    return cc.StreamData(csr, v, O, _z(v, O))


def chain_bound(case, data):
    return cc.chain_bound(case, data) if case.family == "G" else np.zeros((case.B, case.N))


def consts(case, n_ent=None):
    """(t0, dt) as the host forms them, float32."""
    return bc.constants(n_ent or case.N, case.eps)


def scale_of(case):
    """The device scalar scale[0]."""
    return F1 if case.unit_scale else np.float32(GRAD_G) * np.float32(1.0 / (case.B * case.N))


def saturated(z):
    """(p == 1.0f, p == 0.0f) by the kernels' rule; assert_unambiguous makes it unambiguous."""
    return z > SAT_HI, z < -88.0


def assert_unambiguous(case, data):
    z, dz = data.z, chain_bound(case, data)
    lo, hi = z - dz, z + dz
    assert not np.any((hi >= SAT_HI - 0.1) & (lo <= SAT_HI + 0.1)), f"{case.name}: a logit within 0.1 of ln 2^24"
    assert not np.any((hi >= SUB_LO) & (lo <= SUB_HI)), f"{case.name}: a logit inside [{SUB_LO}, {SUB_HI}]"
    if case.family == "S":
        assert np.array_equal(2.0 * z, np.round(2.0 * z)), f"{case.name}: off the lattice"
        assert not np.any(((z > 8.5) & (z < 21.5)) | ((z < -8.5) & (z > -111.5))), f"{case.name}: a level in the gaps"
    else:
        assert np.all(np.abs(z) + dz <= Z_MAX), f"{case.name}: |z| + dz above {Z_MAX}"


def assert_exact(case, data):
    """Families E and S, from the magnitudes: every operand is a small integer multiple of a power of two (hi holds it,
    lo = 0, nothing is an fp16 subnormal after the row's scaling), every partial sum of products, in any order, is an
    integer multiple of the product of the two units below 2^24 of it."""
    v, O = data.v.astype(np.float64), data.O.astype(np.float64)
    units = []
    for X in (v, O):
        q = 2.0 ** math.floor(math.log2(np.abs(X[X != 0]).min()))
        i = X / q
        assert np.array_equal(i, np.round(i)) and np.abs(i).max() < 2 ** 11, f"{case.name}: more than 11 significant bits"
        assert np.abs(i).max(axis=1).max() < 2 ** 14, f"{case.name}: an element below 2^-14 of its row maximum"
        units.append(q)
    assert (np.abs(v) @ np.abs(O).T).max() / (units[0] * units[1]) < 2 ** 24, f"{case.name}: a partial sum may round"
    assert np.array_equal(data.z.astype(np.float32).astype(np.float64), data.z)


def positives_mask(case, csr, mutant=None):
    P = np.zeros((case.B, case.N), dtype=bool)
    for d in range(case.B):
        l = csr.list_of(d)
        if mutant == "first_128_positives_only":
            l = l[:128]
        P[d, l[(l >= 0) & (l < case.N)]] = True
    return P


# ---------------------------------------------------------------------------------------------- reference -
def _logs(z, clamp=True):
    s1, s0 = saturated(z)
    lp, lq = -np.logaddexp(0.0, -z), -np.logaddexp(0.0, z)
    if clamp:
        lp, lq = np.where(s0, -100.0, np.where(s1, 0.0, lp)), np.where(s1, -100.0, np.where(s0, 0.0, lq))
    return lp, lq


def reference(case, data, mutant=None, cuts=None):
    """float64 dict(rows (B,), dv (B, c), gO (N, c)): the sum (rows, dv) and the concatenation (gO) over the blocks of
    `cuts` (None: the whole matrix as one block), which is the whole-matrix result unless the mutant is a block one.

    mutant: saturated_x_kept (x = p - t0 on a saturated element), saturated_positive_kept (-dt on a saturated positive),
    positive_without_negative_term (the correction is -dt ln p), no_t0_in_x, local_smoothing (t0 = eps / n_local),
    positive_in_other_block_counted (an entry outside the block lands on row id % n_local), column_past_N (column
    N - 1 once more in rows and dv), query_past_B (query B - 1 once more in gO), x_lo_dropped / O_lo_dropped /
    sv_lo_dropped (an operand of a tile product rounded to fp16), scatter_slot_minus_one (the row without a list
    scatters the first list of two or more), log_not_clamped (the logs of a saturated element are the float64 ones),
    first_128_positives_only."""
    B, N = case.B, case.N
    csr = data.csr
    cuts = cuts or (0, N)
    O64, v64 = data.O.astype(np.float64), data.v.astype(np.float64)
    sv = float(scale_of(case)) * v64
    P = positives_mask(case, csr, mutant)
    Od, svd = O64, sv
    if mutant == "O_lo_dropped":
        up = 2.0 ** cc.pack_shift(np.abs(data.O).max())
        Od = (O64 * up).astype(np.float16).astype(np.float64) / up
    if mutant == "sv_lo_dropped":
        up = 2.0 ** cc.pack_shift(np.abs(sv).max())
        svd = (sv * up).astype(np.float16).astype(np.float64) / up
    rows, dv, gO = np.zeros(B), np.zeros((B, case.c)), []
    for a, b in zip(cuts[:-1], cuts[1:]):
        t0, dt = [float(x) for x in consts(case, b - a if mutant == "local_smoothing" else N)]
        z = data.z[:, a:b]
        Pb = P[:, a:b].copy()
        if mutant == "positive_in_other_block_counted":
            for d in range(B):
                t = np.nonzero(P[d])[0]
                Pb[d, t[(t < a) | (t >= b)] % (b - a)] = True
        s1, s0 = saturated(z)
        sat = s1 | s0
        lp, lq = _logs(z, clamp=mutant != "log_not_clamped")
        corr = dt * (lp if mutant == "positive_without_negative_term" else lp - lq)
        term = t0 * lp + (1.0 - t0) * lq
        rows -= term.sum(axis=1) + np.where(Pb, corr, 0.0).sum(axis=1)
        p = sc.sigmoid64(z)
        if mutant == "saturated_x_kept":
            x = np.where(s1, 1.0, np.where(s0, 0.0, p)) - t0
        else:
            x = np.where(sat, 0.0, p - (0.0 if mutant == "no_t0_in_x" else t0))
        y = np.where(Pb if mutant == "saturated_positive_kept" else Pb & ~sat, dt, 0.0)
        yg = y
        if mutant == "scatter_slot_minus_one":
            s = int(np.argmax(np.diff(csr.ptr) >= 2))
            l = csr.obj[csr.ptr[s]:csr.ptr[s + 1]]
            l = l[(l >= a) & (l < b)] - a
            yg = y.copy()
            for d in np.nonzero(csr.slot < 0)[0]:
                yg[d, l] = np.where(sat[d, l], 0.0, dt)
        xm = (x * 16384.0).astype(np.float16).astype(np.float64) / 16384.0 if mutant == "x_lo_dropped" else x
        dv += xm @ Od[a:b] - y @ O64[a:b]
        g = xm.T @ svd - yg.T @ sv
        if mutant == "column_past_N" and b == N:
            rows -= term[:, -1]
            dv += np.outer(x[:, -1], O64[N - 1])
        if mutant == "query_past_B":
            g += np.outer(x[B - 1], sv[B - 1])
        gO.append(g)
    return dict(rows=rows, dv=dv, gO=np.concatenate(gO, axis=0))


def bounds(case, data, fast):
    """The whole-matrix reference with its per-element bounds: dict(rows, dv, gO, rows_b, dv_b, gO_b, ...)."""
    B, N = case.B, case.N
    csr = data.csr
    t0, dt = [float(x) for x in consts(case)]
    ref = reference(case, data)
    z, dz = data.z, chain_bound(case, data)
    s1, s0 = saturated(z)
    live = ~(s1 | s0)
    p, q = sc.sigmoid64(z), sc.sigmoid64(-z)
    darg = (ARG * np.abs(z) + (2 if fast else 2 * sc.EXPF_ULP)) * U
    dp = np.where(live, 1.01 * p * q * (darg + dz) + (3 if fast else 2) * U * p, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rp, rq = np.where(live, dp / p, 0.0), np.where(live, (dp + U * q) / q, 0.0)
    assert rp.max() < 1.0 and rq.max() < 1.0, f"{case.name}: a probability error as large as p or 1 - p"
    Lp, Lq = -np.log1p(-rp), -np.log1p(-rq)
    lp, lq = _logs(z)
    alp, alq = np.abs(lp), np.abs(lq)
    mag = t0 * alp + (1.0 - t0) * alq
    neg = t0 * (Lp + 4 * U * alp * live) + U * t0 * alp + (1.0 - t0) * (Lq + 4 * U * alq * live) + 2 * U * (1.0 - t0) * alq \
        + (1 + 16 * 1.01) * U * mag
    P = positives_mask(case, csr)
    n = csr.stored()
    pmag = np.where(P, dt * np.abs(lp - lq), 0.0)
    pos = np.where(P, dt * (Lp + Lq + 4 * U * (alp + alq) * live), 0.0) + 2 * U * pmag
    rows_b = neg.sum(axis=1) + pos.sum(axis=1) + (-(-n // 128) + 10) * U * pmag.sum(axis=1) \
        + 2.0 ** -50 * (mag.sum(axis=1) + pmag.sum(axis=1))
    # the backward: ce_kernel_cases.stream_backward's terms with the BCE dx
    x = np.where(live, p - t0, 0.0)
    dx = np.where(live, dp + U * np.abs(x), 0.0)
    O64 = data.O.astype(np.float64)
    sv = float(scale_of(case)) * data.v.astype(np.float64)
    ax, aO, asv = np.abs(x), np.abs(O64), np.abs(sv)
    r_j, r_d = cc._term_roundings(case)
    Pl = (P & live).astype(np.float64)
    chain = (32 * -(-n // 128) + 6).astype(np.float64)
    dv_floor = 2.0 ** -39 * (aO.sum(axis=0)[None, :] + aO.max() * ax.sum(axis=1)[:, None])
    dv_sweep = dx @ aO + 3 * U22 * (ax @ aO) + U * ((ax * r_j[None, :]) @ aO)
    dv_b = dv_sweep + dv_floor + (chain * U * dt)[:, None] * (Pl @ aO) + 2 * U * np.abs(ref["dv"])
    m_j = Pl.sum(axis=0)
    gO_floor = 2.0 ** -39 * (asv.sum(axis=0)[None, :] + asv.max() * ax.sum(axis=0)[:, None])
    gO_sweep = dx.T @ asv + (3 * U22 + U) * (ax.T @ asv) + U * ((ax * r_d[:, None]).T @ asv)
    gO_b = gO_sweep + gO_floor + ((m_j + 6) * U * dt)[:, None] * (Pl.T @ asv) + 2 * U * np.abs(ref["gO"])
    quiet_q = ~live.any(axis=1)                               # every column saturated (so every positive too)
    quiet_e = ~live.any(axis=0)
    return dict(ref, rows_b=rows_b, dv_b=dv_b, gO_b=gO_b, quiet_q=quiet_q, quiet_e=quiet_e, dv_floor=dv_floor,
                gO_floor=gO_floor, dv_sweep=dv_sweep, gO_sweep=gO_sweep, dv_mass=ax @ aO, gO_mass=ax.T @ asv)


def verdict(ref, got_rows, got_dv, got_gO):
    """-> (largest error / bound of rows, of dv, of gO); inf for a non-finite output, for a non-zero bit in the dv row of
    a query without an unsaturated element, for a gO row that no unsaturated element touches and is not +0.0."""
    if not (np.isfinite(got_rows).all() and np.isfinite(got_dv).all() and np.isfinite(got_gO).all()):
        return np.inf, np.inf, np.inf
    r_rows = cc._ratio(np.abs(got_rows - ref["rows"]), ref["rows_b"])
    r_dv = cc._ratio(np.abs(got_dv.astype(np.float64) - ref["dv"]), ref["dv_b"])
    r_gO = cc._ratio(np.abs(got_gO.astype(np.float64) - ref["gO"]), ref["gO_b"])
    if np.any(np.ascontiguousarray(got_dv, dtype=np.float32)[ref["quiet_q"]].view(np.uint32) != 0):
        r_dv = np.inf
    if np.any(np.ascontiguousarray(got_gO, dtype=np.float32)[ref["quiet_e"]].view(np.uint32) != 0):
        r_gO = np.inf
    return r_rows, r_dv, r_gO


# ---------------------------------------------------------------------------------------------- emulation -
def logistic32(z32, fast, perturb=0):
    """The two logistics in numpy fp32; perturb = +-1 moves every (finite, non-zero) exponential by one ulp."""
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2((z32 * NL2E32).astype(np.float32)) if fast else np.exp(-z32)
        e = e.astype(np.float32)
        if perturb:
            moved = np.nextafter(e, np.float32(np.inf) if perturb > 0 else F0).astype(np.float32)
            e = np.where(np.isfinite(e) & (e > 0), moved, e)
        return (F1 / (F1 + e)).astype(np.float32)


def clog32(y):
    """rtk_clog on a normal or zero argument."""
    with np.errstate(divide="ignore"):
        return np.maximum((np.log2(y.astype(np.float32)).astype(np.float32) * LN2_32).astype(np.float32), np.float32(-100.0))


def emul(case, data, fast, perturb=0):
    """The link in numpy fp32 from the fp32 logit: rows (float64; sixteen fp32 adds per lane and tile, float64 across),
    dv and gO (float32; the 2^14 hi/lo split of x, three fp32 products against the hi/lo split of O and of scale v)."""
    B, N = case.B, case.N
    t0, dt = consts(case)
    p = logistic32(data.z.astype(np.float32), fast, perturb)
    lp, lq = clog32(p), clog32(F1 - p)
    term = ((t0 * lp).astype(np.float32) + ((F1 - t0) * lq).astype(np.float32)).astype(np.float32)
    T = -(-N // 32)
    pad = np.zeros((B, 32 * T), dtype=np.float32)
    pad[:, :N] = term
    grp = pad.reshape(B, T, 4, 2, 4).transpose(0, 1, 3, 2, 4).reshape(B, T, 2, 16)      # row 8 g + 4 h + q of the tile
    ls = np.zeros((B, T, 2), dtype=np.float32)
    for i in range(16):
        ls = (ls + grp[..., i]).astype(np.float32)
    rows = -ls.astype(np.float64).sum(axis=(1, 2))
    P = positives_mask(case, data.csr)
    corr = (dt * (lp - lq).astype(np.float32)).astype(np.float32)
    for d in range(B):
        rows[d] -= float(corr[d, P[d]].sum(dtype=np.float32))
    sat = (p == F1) | (p == F0)
    x = np.where(sat, F0, (p - t0).astype(np.float32)).astype(np.float32)
    Y = np.where(P & ~sat, dt, F0).astype(np.float32)
    xh, xl = cc._split16(x * np.float32(16384.0))

    def product(A_h, A_l, M):
        sh = cc.pack_shift(np.abs(M).max())
        th, tl = cc._split16((M * np.float32(2.0 ** sh)).astype(np.float32))
        acc = (A_h @ th + A_h @ tl + A_l @ th).astype(np.float32)
        return (acc * np.float32(2.0 ** (-14 - sh))).astype(np.float32)

    sv = (data.v * scale_of(case)).astype(np.float32)
    dv = product(xh, xl, data.O) - (Y @ data.O).astype(np.float32)
    gO = product(xh.T.copy(), xl.T.copy(), sv) - (Y.T @ sv).astype(np.float32)
    return rows, dv, gO


def smoothing_miss_factor(part=MUTANT_PART):
    """By how much a block form with t0 = eps / n_local leaves the doubled bound on the small case: the largest of
    (rows, dv, gO), over both logistics the smaller."""
    data = operands(part.case)
    m = reference(part.case, data, "local_smoothing", part.cuts)
    out = []
    for fast in (False, True):
        ref = bounds(part.case, data, fast)
        out.append(max(verdict(ref, m["rows"], m["dv"].astype(np.float32), m["gO"].astype(np.float32))) / 2.0)
    return min(out)
