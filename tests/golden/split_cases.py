"""A numpy model of the split-fp16 score kernels (rtk_score_packed_f32: cg, ws, v3) and operands on which the model is
EXACT, so that a kernel has to return it bit for bit whatever its summation order.  numpy only.

The split is deterministic arithmetic (csrc/rtk_pack.h, and the O-side conversion of each kernel):
    sh = pack_shift(row max)        power of two that brings the row maximum into [2^14, 2^15)
    hi = fp16(x 2^sh)               round to nearest even
    lo = fp16(x 2^sh - hi)          (x 2^sh - hi is exact in fp32)
and v_mfma_f32_32x32x16_f16 forms exact products of fp16 values, so
    z_model[d, j] = (vh.oh + vh.ol + vl.oh) 2^-(sh_v[d] + sh_o[j])
is the header's formula with the vl.ol term dropped.  How the matrix core rounds or orders its adds is not documented;
the exact families do not depend on it: every product of a case is a multiple of a power of two g and, per output, the
sum of the absolute values of the 3 c products is at most 2^23 g (asserted, assert_exact) -- every partial sum, in any
order, is then an fp32 number (one bit of headroom under fp32's 24) and no add can round.

Families (all exact; each pins something else):
    fewbit   elements 0, +-(12288 + b), +-(16384 + 2|b|), b = -3..3, in units of the row's power of two: hi = 12288 or
             16384, lo = b or 2|b| -- both lo planes populated, signs mixed, zeros present; row scales spread |z| over
             about 2^-6 .. 128 (the logistic's whole range)
    tail     ONE maximal element per row, at k = c - 1, k = 0 or in the second k-half of the last k-step, every other
             element a quarter as large ((12288 + b) / 4): a row maximum that misses the element shifts the row by two more
             bits and the element overflows fp16.  Every fifth O row is 2^27 larger than the row before it: a k tail read
             from the next row moves the shift by more than the lo plane can follow
    shift    row maxima exactly 2^k, (2 - 2^-23) 2^k (its scaled value rounds to fp16 2^15), 2^k (1 + 2^-23); an
             all-zero row, a row of -0.0, a row with one non-zero element; on both sides
    scale    fewbit rows with row exponents over {-60, -40, 0, 40, 60}^2; outputs whose unit or abs-sum leaves fp32's
             normal range are masked out (Case.valid)
    sublo15  elements at 2^-15 and 2^-16 of their row's maximum facing maximal elements, 22 significant bits: hi and lo
             are normal fp16 numbers and the split keeps every bit
    sublo    the same at 2^-17 .. 2^-26 with 24-bit mantissas: lo is an fp16 subnormal (one bit less per factor of two)
             or zero.  Kept apart from everything else: if the matrix core treats fp16 subnormal operands otherwise
             than the model does, it shows here and nowhere else
Every case's O lies in a buffer (Case.obuf) with o_off floats in front of it and one row behind it that hold GUARD, a
huge fewbit value: a kernel that reads past c, past row N - 1 or in front of a misaligned base changes a bit.

The real layer (real_case) is compared with the model under |z - z_model| <= gamma(48 KS) T 2^-(sh_v + sh_o): 3 * 16 * KS
terms in one chain (+ 3 for the adds of a fifth group's four chains), gamma as in exact_cases.py.
"""
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from exact_cases import gamma

F32, F16, F64 = np.float32, np.float16, np.float64
FAMILIES = ("fewbit", "tail", "shift", "scale", "sublo15", "sublo")
CAP = 2.0 ** 23                       # max T / g per output
GUARD = F32(16390.0 * 2.0 ** 40)      # what lies around O in its buffer
SCALE_EXPS = (-60, -40, 0, 40, 60)

# ---- probabilities: relative bounds from the per-step accuracies the header states ------------------------------
# fast form: t = fl(z * fl(-log2 e)) (two roundings, 2^-24 each, relative to t: 2^-23 |t| ln 2 = 2^-23 |z| in the result's
# relative error, ln 2 * log2 e = 1), v_exp_f32 (1 ulp = 2^-23), one add (2^-24), v_rcp_f32 (1 ulp = 2^-23):
#     |dp| / p <= 2^-23 (|z| + 2.5).  (ws and cg fold the row factors, powers of two, into the constant first.)
# exact form: ocml expf at e ulp, one add, an IEEE divide: 2^-24 (2 e + 2).  e = 3: the OpenCL limit for exp, taken
# in place of a figure for this ROCm's expf (the library's own comment in rtk_common.h says <= 1 ulp).
EXPF_ULP = 3
P_FLOOR = 2.0 ** -126                 # results the hardware returns as zero (no subnormal from v_rcp_f32 / an overflowed exp)


def p_bound(z, fast):
    p = sigmoid64(z)
    rel = 2.0 ** -23 * (np.abs(z) + 2.5) if fast else 2.0 ** -24 * (2 * EXPF_ULP + 2) * np.ones_like(z)
    return rel * p + P_FLOOR


def sigmoid64(z):
    z = np.asarray(z, dtype=F64)
    with np.errstate(over="ignore"):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


# ---- the model ------------------------------------------------------------------------------------------------------
def pack_shift(mx):
    """rtk_pack_shift: 14 - floor(log2 mx) by frexp, clamped to +-100; 0 for mx <= 0 or a non-finite mx."""
    mx = np.asarray(mx, dtype=F32)
    ok = (mx > 0) & np.isfinite(mx)
    _, e = np.frexp(np.where(ok, mx, F32(1)))
    return np.where(ok, np.clip(14 - (e.astype(np.int64) - 1), -100, 100), 0).astype(np.int64)


def split(X, bound=None, shift=pack_shift, round_hi=None):
    """(hi, lo, sh) of the rows of X as the kernels form them, in float32 / float16.  bound: a magnitude (scalar or per
    row) to take the shift from in place of the row maximum (a later GEMM test passes its global bound).  shift and
    round_hi exist for the mutants."""
    X = np.ascontiguousarray(X, dtype=F32)
    mx = np.fmax.reduce(np.abs(X), axis=1, initial=F32(0)) if bound is None else np.broadcast_to(F32(bound), X.shape[:1])
    sh = shift(mx)
    with np.errstate(over="ignore", invalid="ignore"):
        y = X * np.ldexp(F32(1), sh).astype(F32)[:, None]
        hi = y.astype(F16) if round_hi is None else round_hi(y)
        lo = (y - hi.astype(F32)).astype(F16)
    return hi, lo, sh


Planes = namedtuple("Planes", "vh vl shv oh ol sho")      # float64 values of the fp16 planes, int64 shifts
Model = namedtuple("Model", "z T ll acc Tacc shv sho")


def planes(v, O, **kw):
    vh, vl, shv = split(v, **kw)
    oh, ol, sho = split(O, **kw)
    return Planes(vh.astype(F64), vl.astype(F64), shv, oh.astype(F64), ol.astype(F64), sho)


def ksteps(c):
    return (c + 15) // 16


def fifth_ranges(KS):
    """k-step ranges of the four chains of a fifth-group column (rtk_score_cg_kernel.h: s_begin / s_end)"""
    return [((KS * w + 3) // 4, (KS * (w + 1) + 3) // 4) for w in range(4)]


def _chain(P, k0=None, k1=None, cols=None):
    sl = slice(k0, k1)
    oh, ol = (P.oh, P.ol) if cols is None else (P.oh[cols], P.ol[cols])
    return P.vh[:, sl] @ (oh[:, sl] + ol[:, sl]).T + P.vl[:, sl] @ oh[:, sl].T      # oh + ol is exact in float64


def accumulate(P, fifth=None, skip=None):
    """vh.oh + vh.ol + vl.oh in float64, unscaled.  Columns of `fifth` (bool mask): the same sum cut into the cg kernel's
    four k-step ranges and added in that order.  skip = (w, ks): that k-step is missing from range w (a mutant)."""
    acc = _chain(P)
    if fifth is not None and fifth.any():
        c = P.vh.shape[1]
        cols = np.flatnonzero(fifth)
        tot = None
        for w, (s0, s1) in enumerate(fifth_ranges(ksteps(c))):
            part = np.zeros((P.vh.shape[0], cols.size))
            for ks in range(s0, s1):
                if skip == (w, ks):
                    continue
                part = part + _chain(P, 16 * ks, min(16 * ks + 16, c), cols)
            tot = part if tot is None else tot + part
        acc[:, cols] = tot
    return acc


def unscale(acc, shv, sho):
    return np.ldexp(acc, -(shv[:, None] + sho[None, :]))


def score_model(v, O, fifth=None, P=None):
    """z_model, the abs-sum matrix T and the dropped term ll = vl.ol (all float64, unscaled); acc / Tacc: the first two
    in the accumulator's units (before the row factors)."""
    P = P or planes(v, O)
    acc = accumulate(P, fifth)
    Tacc = np.abs(P.vh) @ (np.abs(P.oh) + np.abs(P.ol)).T + np.abs(P.vl) @ np.abs(P.oh).T
    ll = P.vl @ P.ol.T
    return Model(unscale(acc, P.shv, P.sho), unscale(Tacc, P.shv, P.sho), unscale(ll, P.shv, P.sho), acc, Tacc, P.shv, P.sho)


def z_bound(m, c, fifth=None):
    """real layer: gamma(48 KS) T, 3 more roundings on the fifth group's columns"""
    n = np.full(m.T.shape[1], 48.0 * ksteps(c))
    if fifth is not None:
        n = n + 3.0 * fifth
    return gamma(n)[None, :] * m.T


def _lsb_exp(x):
    """per column k: the exponent of the lowest set bit over the non-zero entries of x[:, k] (fp16 values); a column
    of zeros: a large number"""
    m, e = np.frexp(np.abs(x))
    n = (m * 2048.0).astype(np.int64)          # 11 significant bits at the most
    assert np.array_equal(n / 2048.0, m)
    tz = np.log2(np.maximum(n & -n, 1).astype(F64)).astype(np.int64)
    return np.where(x != 0, e - 11 + tz, 10 ** 6).min(axis=0)


def product_unit(P):
    """g: the largest power of two that divides every product of the three terms, in accumulator units.  Every query
    row meets every entity row, so column k of a v plane multiplies exactly column k of an O plane."""
    lv, lvl, lo_, lol = _lsb_exp(P.vh), _lsb_exp(P.vl), _lsb_exp(P.oh), _lsb_exp(P.ol)
    e = min((lv + lo_).min(), (lv + lol).min(), (lvl + lo_).min())
    return 2.0 ** int(e) if e < 10 ** 5 else 1.0


def split_residual(X):
    """(y, dy): the scaled rows x 2^sh and what hi + lo miss of them (float64; zero unless lo was rounded)"""
    hi, lo, sh = split(X)
    y = np.ldexp(np.asarray(X, dtype=F64), sh[:, None])
    return y, y - hi.astype(F64) - lo.astype(F64), sh


def assert_exact(case, m=None):
    """The criterion of an exact case.  Returns (m, headroom = max T / g)."""
    m = m or score_model(case.v, case.O, case.fifth)
    P = case.P if case.P is not None else planes(case.v, case.O)
    ok = case.valid if case.valid is not None else np.ones(m.z.shape, dtype=bool)
    assert np.isfinite(m.acc).all(), case.name
    g = case.g or product_unit(P)
    head = float(m.Tacc.max() / g)
    assert head <= CAP, f"{case.name}: max T / g = 2^{np.log2(head):.2f} > 2^23"
    assert np.array_equal(m.acc / g, np.rint(m.acc / g)), case.name
    with np.errstate(over="ignore"):
        z32 = m.z.astype(F32)
    assert np.array_equal(z32.astype(F64)[ok], m.z[ok]) and np.isfinite(z32[ok]).all(), f"{case.name}: z_model is not fp32"
    assert (np.abs(m.z[ok])[m.z[ok] != 0] >= 2.0 ** -126).all(), case.name
    # z_model + vl.ol is the float64 product of the fp32 operands, up to what a ROUNDED lo plane misses (sublo only)
    z64 = case.v.astype(F64) @ case.O.astype(F64).T
    yv, dv, shv = split_residual(case.v)
    yo, do, sho = split_residual(case.O)
    if case.family != "sublo":
        assert not dv.any() and not do.any(), f"{case.name}: hi + lo does not hold the operand"
    if dv.any() or do.any():
        slack = unscale(np.abs(dv) @ np.abs(yo).T + np.abs(yv) @ np.abs(do).T, shv, sho)
        same = np.abs(z64 - (m.z + m.ll)) <= slack * (1 + 2.0 ** -40)
    else:
        same = z64 == m.z + m.ll
    assert same[ok].all(), f"{case.name}: z_model + ll != float64 product"
    return m, head


# ---- shapes -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    N: int
    c: int
    B: int
    pitch: int = 0          # 0: dense rows
    o_off: int = 0          # floats in front of O's 16-byte-aligned base
    note: str = ""

    @property
    def id(self):
        return f"N{self.N}-c{self.c}-B{self.B}" + (f"-p{self.pitch}" if self.pitch else "") + (f"-off{self.o_off}" if self.o_off else "")

    @property
    def ld(self):
        return self.pitch or self.N

    @property
    def kernels(self):
        """hints this shape can run on (a cg or ws hint falls through to v3 elsewhere)"""
        vec = self.c % 4 == 0 and self.c <= 208 and self.o_off == 0
        return ("cg", "ws", "v3") if vec else ("v3",)


def _s(N, c, B, pitch=0, o_off=0, note=""):
    return Shape(N, c, B, pitch, o_off, note)


SHAPES = [
    # the shapes of test_gpu_score_cg.py (B cut to <= 64 at the two 40 943-entity shapes)
    _s(40943, 200, 64, 40960, note="the bench workload: 1280 groups = 5 per workgroup, nontemporal stores"),
    _s(40943, 200, 50, note="dense rows, ragged last query tile"),
    _s(20000, 200, 64, note="625 groups in 256 sets of 2 and 3"),
    _s(36000, 64, 40, note="sets of 4 and 5 side by side"),
    _s(2000, 200, 64, note="63 groups, one per workgroup"),
    _s(333, 36, 70, note="KS = 3: two M waves with an empty k-range; N % 32 != 0"),
    _s(100, 4, 5, note="KS = 1, last group 4 columns wide"),
    _s(20, 8, 33, note="fewer entities than one group"),
    _s(167, 208, 96, 192, note="KS = 13 at the widest c; 128-byte rows"),
    _s(100000, 64, 40, note="3125 groups: three sets per workgroup; ws: whole tiles + remainder"),
    _s(5 * 32 * 256 + 1, 16, 32, note="one group more than a single pass holds: two passes"),
    # v3: KS in {1, 13, 14, 16, 17, 32}, B in {1, 33, 70}, N % 128 in {0, 1, 127}
    _s(384, 16, 1, note="v3 KS = 1, B = 1, N % 128 == 0"),
    _s(257, 208, 33, note="v3 KS = 13, N % 128 == 1"),
    _s(383, 224, 70, note="v3 KS = 14 (the first c past the cg / ws kernels), N % 128 == 127"),
    _s(300, 256, 33, note="v3 KS = 16: two workgroups per CU for the last time"),
    _s(259, 272, 70, 320, note="v3 KS = 17: one workgroup per CU; padded pitch"),
    _s(200, 512, 33, note="v3 KS = 32"),
    _s(333, 36, 33, o_off=1, note="c % 16 = 4, O one float off its alignment: scalar loads at c % 4 == 0"),
    _s(511, 200, 70, o_off=1, note="c % 16 = 8, misaligned O"),
    _s(300, 7, 33, note="c % 4 != 0: scalar loads, KS = 1"),
    _s(385, 97, 70, note="c % 4 != 0, c % 16 = 1"),
    _s(130, 509, 33, note="c % 4 != 0 at KS = 32, c % 16 = 13"),
    _s(4100, 16, 520, note="v3: 33 x 17 = 561 units on a 512-workgroup grid"),
]
SHAPE_IDS = [s.id for s in SHAPES]


# ---- cases ------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    shape: Shape
    v: np.ndarray           # (B, c) fp32
    obuf: np.ndarray        # o_off + (N + 1) c fp32: GUARD, O, GUARD
    valid: np.ndarray = None   # (B, N) bool: outputs that are compared (None: all)
    fifth: np.ndarray = None   # (N,) bool: fifth-group columns of the kernel the model is for (set by the tests)
    model: object = None       # score_model(v, O) without a fifth group, from the generator
    P: object = None           # planes(v, O)
    g: float = None            # product_unit(P)

    @property
    def O(self):
        s = self.shape
        return self.obuf[s.o_off:s.o_off + s.N * s.c].reshape(s.N, s.c)

    @property
    def guard_row(self):
        s = self.shape
        return self.obuf[s.o_off + s.N * s.c:]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _fewbit_rows(rng, R, c, density, low=1.0):
    """rows of 0, +-(12288 + b) * low and (at least one per row) +-(16384 + 2|b|), in accumulator units"""
    b = rng.integers(-3, 4, size=(R, c))
    big = rng.random((R, c)) < 0.3
    y = np.where(big, 16384 + 2 * np.abs(b), 12288 + b).astype(F64)
    y *= rng.choice([-1.0, 1.0], size=(R, c)) * (rng.random((R, c)) < density)
    if low != 1.0:      # tail: the maximal element is set by the caller, everything else is `low` as large
        y = np.where(big, 0.0, y) * low
    else:
        k = rng.integers(0, c, size=R)
        y[np.arange(R), k] = rng.choice([-1.0, 1.0], size=R) * (16384 + 2 * rng.integers(0, 4, size=R))
    return y


def _tail_positions(c):
    """where a tail row's only maximal element sits: k = c - 1, k = 0, the second k-half of the last k-step (of the
    one before it when the last k-step has no second half; nowhere at c <= 8)"""
    pos = [c - 1, 0]
    k2 = 16 * (ksteps(c) - 1) + 8
    if k2 < c:
        pos.append(k2 + (c - 1 - k2) // 2)
    elif c > 8:         # c % 16 in 1..8: the last k-step has no second half -- the one before it has
        pos.append(k2 - 16 + 5)
    return pos


def _to_rows(y, e):
    """accumulator units -> fp32 operand rows: row r is y[r] * 2^(e[r] - 14) (exact)"""
    x = np.ldexp(y, (np.asarray(e) - 14)[:, None])
    x32 = x.astype(F32)
    assert np.array_equal(x32.astype(F64), x)
    return x32


def _sublo_rows(rng, R, c, kmax, ktiny, ks):
    """row maximum exactly 2^14 at column kmax; one element m 2^(14 - k) at column ktiny, k cycling through ks by row:
    22 and 21 significant bits at k = 15 and 16, 24 below"""
    y = np.zeros((R, c))
    y[:, kmax] = rng.choice([-1.0, 1.0], size=R) * 16384.0
    k = np.asarray(ks)[np.arange(R) % len(ks)]
    bits = np.where(k <= 16, 36 - k, 23)         # the element's last place: 2^-22 of the unit at k = 15, 16
    m = 1.0 + ((rng.integers(0, 2 ** 23, size=R) >> (23 - bits)) | 1) * 2.0 ** -bits.astype(F64)   # the last bit set
    y[:, ktiny] = rng.choice([-1.0, 1.0], size=R) * np.ldexp(m, 14 - k)
    return y


_SHIFT_FILL = np.array([0.0, 0.0, 8192.0, -8192.0, 4096.0, -4096.0, 6144.0, -6144.0])


def _shift_rows(rng, R, c, k_exact, k_odd, k_dead):
    """six kinds of row, cycling: maximum exactly 2^14 (at column k_exact); (2 - 2^-23) 2^14 and (1 + 2^-23) 2^14 (at
    k_odd: the other operand is zero there, a product with their lo = -+2^-9 could not meet the cap); all zero; all
    -0.0; one non-zero element.  The rest: sparse coarse values with lo = 0.  Column k_dead (the other operand's
    k_odd) is zero."""
    y = _SHIFT_FILL[rng.integers(0, len(_SHIFT_FILL), size=(R, c))]
    y[:, k_dead] = 0.0
    y[:, k_odd] = 0.0
    kind = np.arange(R) % 6
    sgn = rng.choice([-1.0, 1.0], size=R)
    y[kind == 0, k_exact] = sgn[kind == 0] * 16384.0
    y[kind == 1, k_odd] = sgn[kind == 1] * (2.0 - 2.0 ** -23) * 16384.0
    y[kind == 2, k_odd] = sgn[kind == 2] * (1.0 + 2.0 ** -23) * 16384.0
    y[kind == 3] = 0.0
    y[kind == 4] = -0.0
    y[kind == 5] = 0.0
    y[kind == 5, k_exact] = sgn[kind == 5] * 24576.0
    # kinds 1 and 2 keep a true maximum: their fill stays below 2^14; kind 0 rows may hold +-8192 only
    return y


def make_case(shape, family):
    """The exact case of a family on a shape.  Densities are lowered until max T / g <= 2^23 (never the cap raised)."""
    assert family in FAMILIES
    N, c, B = shape.N, shape.c, shape.B
    name = f"{family}/{shape.id}"
    density = 0.5
    for _ in range(12):
        rng = _rng(name)
        valid = None
        if family in ("fewbit", "scale"):
            yv, yo = _fewbit_rows(rng, B, c, density), _fewbit_rows(rng, N, c, density)
            if family == "fewbit":      # |z| ~ 2^2 * 2^(ev + eo) at c = 200: 2^-6 .. 2^6 and the tails beyond
                top = 3 if c >= 64 else (4 if c >= 16 else 5)
                ev, eo = rng.integers(-4, top, size=B), rng.integers(-4, top, size=N)
            else:
                ev = np.asarray(SCALE_EXPS)[np.arange(B) % 5]            # the row maximum lies in [2^e, 2^(e + 1))
                eo = np.asarray(SCALE_EXPS)[(np.arange(N) // 3) % 5]
        elif family == "tail":
            pos = _tail_positions(c)
            yv, yo = _fewbit_rows(rng, B, c, density, 0.25), _fewbit_rows(rng, N, c, density, 0.25)
            for y in (yv, yo):
                R = y.shape[0]
                k = np.asarray(pos)[np.arange(R) % len(pos)]
                y[np.arange(R), k] = rng.choice([-1.0, 1.0], size=R) * (16384 + 2 * rng.integers(0, 4, size=R))
            ev = rng.integers(-4, 3, size=B)
            eo = rng.integers(-4, 3, size=N) + 27 * (np.arange(N) % 5 == 1)
        elif family == "shift":
            yv, yo = _shift_rows(rng, B, c, 0, 2, 3), _shift_rows(rng, N, c, 1, 3, 2)
            ev, eo = rng.integers(-30, 31, size=B), rng.integers(-30, 31, size=N)
        else:
            ks = (15, 16) if family == "sublo15" else tuple(range(17, 27))
            yv, yo = _sublo_rows(rng, B, c, c - 1, 0, ks), _sublo_rows(rng, N, c, 0, c - 1, ks)
            ev, eo = rng.integers(-4, 3, size=B) + 10, rng.integers(-4, 3, size=N) + 10
        v, O = _to_rows(yv, ev), _to_rows(yo, eo)
        obuf = np.full(shape.o_off + (N + 1) * c, GUARD, dtype=F32)
        obuf[shape.o_off:shape.o_off + N * c] = O.ravel()
        case = Case(name, family, shape, v, obuf, valid)
        P = planes(v, O)
        m = score_model(v, O, P=P)
        g = product_unit(P)
        if family == "scale":           # keep the outputs whose unit and abs-sum are normal fp32 numbers
            case.valid = (np.ldexp(g, -(m.shv[:, None] + m.sho[None, :])) >= 2.0 ** -126) & (m.T < 2.0 ** 127)
        if m.Tacc.max() / g <= CAP:
            case.model, case.P, case.g = m, P, g
            return case
        density *= 0.8
    raise AssertionError(f"{name}: no density meets the cap")


def real_case(shape, kind):
    """Real-valued operands: 'rows' = normals times per-row powers of two over 2^-6 .. 2^6; 'range' = a within-row
    range of 2^0 .. 2^24."""
    N, c, B = shape.N, shape.c, shape.B
    name = f"real-{kind}/{shape.id}"
    rng = _rng(name)

    def rows(R):
        x = rng.standard_normal((R, c))
        if kind == "rows":
            return (x * 2.0 ** rng.integers(-6, 7, size=(R, 1))).astype(F32)
        return (x * 2.0 ** rng.uniform(0, 24, size=(R, c)) * 2.0 ** -12).astype(F32)

    v, O = rows(B), rows(N)
    obuf = np.full(shape.o_off + (N + 1) * c, GUARD, dtype=F32)
    obuf[shape.o_off:shape.o_off + N * c] = O.ravel()
    return Case(name, "real", shape, v, obuf)


def split_bound(v, O):
    """|z_model - z64| <= |ll| + what the rounding of the lo planes leaves: per element at most half a unit of lo's last
    place, 2^-11 ulp_fp16(hi) / 2 ... bounded here by 2^-11 ulp_fp16(hi) with the subnormal floor 2^-25 (accumulator
    units), times the other operand's magnitude.  The header's normwise statement follows from it."""
    def err(X):
        hi, lo, sh = split(X)
        y = np.ldexp(np.asarray(X, dtype=F64), sh[:, None])
        _, e = np.frexp(np.abs(hi.astype(F64)))
        ulp_hi = np.where(hi != 0, np.ldexp(1.0, np.maximum(e - 11, -24)), 2.0 ** -24)
        return y, np.maximum(2.0 ** -11 * ulp_hi, 2.0 ** -25), sh
    yv, dv, shv = err(v)
    yo, do, sho = err(O)
    m = score_model(v, O)
    return m, np.abs(m.ll) + unscale(dv @ np.abs(yo).T + np.abs(yv) @ do.T + dv @ do.T, shv, sho)


# ---- mutants: each returns a wrong z (float64) for a case ------------------------------------------------------------------
def _pad(x, c16):
    return np.pad(x, ((0, 0), (0, c16 - x.shape[1])))


def _mut_planes(case, **kw):
    return planes(case.v, case.O, **kw)


def _z(P, acc):
    return unscale(acc, P.shv, P.sho)


def m_drop(term):
    def f(case):
        P = _mut_planes(case)
        sub = {"hh": P.vh @ P.oh.T, "hl": P.vh @ P.ol.T, "lh": P.vl @ P.oh.T}[term]
        return _z(P, accumulate(P, case.fifth) - sub)
    return f


def m_add_ll(case):
    P = _mut_planes(case)
    return _z(P, accumulate(P, case.fifth) + P.vl @ P.ol.T)


def m_swap_khalves(case):
    P = _mut_planes(case)
    c16 = 16 * ksteps(case.shape.c)
    sw = lambda x: _pad(x, c16).reshape(x.shape[0], -1, 2, 8)[:, :, ::-1, :].reshape(x.shape[0], c16)
    Q = Planes(sw(P.vh), sw(P.vl), P.shv, _pad(P.oh, c16), _pad(P.ol, c16), P.sho)
    return _z(P, accumulate(Q))


def m_lo_neighbour_row(case):
    P = _mut_planes(case)
    return _z(P, accumulate(P._replace(ol=np.roll(P.ol, -1, axis=0)), case.fifth))


def _o_with_tail(case):
    """O rows widened to 16 KS columns, the k tail read on into the next row (the last row: into the guard row)"""
    s = case.shape
    c16 = 16 * ksteps(s.c)
    flat = np.concatenate([case.obuf[s.o_off:], np.full(c16, GUARD, dtype=F32)])
    idx = np.arange(s.N)[:, None] * s.c + np.arange(c16)[None, :]
    return flat[idx]


def m_tail_from_next_row(case):
    c16 = 16 * ksteps(case.shape.c)
    P = planes(_pad(case.v, c16), _o_with_tail(case))
    return _z(P, accumulate(P))


def m_row_past_n(case):
    """the last column reads the row after the last entity row"""
    O = case.O.copy()
    O[-1] = case.guard_row
    P = planes(case.v, O)
    return _z(P, accumulate(P, case.fifth))


def m_shift_at_pow2(delta):
    def shift(mx):
        sh = pack_shift(mx)
        m, _ = np.frexp(np.asarray(mx, dtype=F32))
        return sh + delta * (m == 0.5)

    def f(case):
        P = _mut_planes(case, shift=shift)
        return _z(P, accumulate(P, case.fifth))
    return f


def m_max_one_khalf(case):
    """the row maximum of O taken over the first k-half of every k-step only"""
    O = case.O
    half = (np.arange(O.shape[1]) % 16) < 8
    mx = np.abs(O[:, half]).max(axis=1)
    vh, vl, shv = split(case.v)
    sho = pack_shift(mx)
    with np.errstate(over="ignore", invalid="ignore"):
        y = O * np.ldexp(F32(1), sho).astype(F32)[:, None]
        oh = y.astype(F16)
        ol = (y - oh.astype(F32)).astype(F16)
    P = Planes(vh.astype(F64), vl.astype(F64), shv, oh.astype(F64), ol.astype(F64), sho)
    with np.errstate(invalid="ignore"):
        return _z(P, accumulate(P))


def m_row_factor_r4(case):
    P = _mut_planes(case)
    return unscale(accumulate(P, case.fifth), np.roll(P.shv, -4), P.sho)


def m_col_factor_neighbour(case):
    P = _mut_planes(case)
    return unscale(accumulate(P, case.fifth), P.shv, np.roll(P.sho, -1))


def m_fifth_missing_kstep(case):
    P = _mut_planes(case)
    KS = ksteps(case.shape.c)
    w = 3 if KS >= 4 else max(i for i, (a, b) in enumerate(fifth_ranges(KS)) if b > a)
    return _z(P, accumulate(P, case.fifth, skip=(w, fifth_ranges(KS)[w][0])))


def _truncate_f16(y):
    hi = y.astype(F16)
    up = np.abs(hi.astype(F32)) > np.abs(y)
    return np.where(up, np.nextafter(hi, F16(0)), hi).astype(F16)


def m_hi_truncated(case):
    P = _mut_planes(case, round_hi=_truncate_f16)
    return _z(P, accumulate(P, case.fifth))


# name -> (function, the family whose cases must catch it, which shapes it applies to)
_ALL = lambda case: True
MUTANTS = {
    "drop vh.oh": (m_drop("hh"), "fewbit", _ALL),
    "drop vh.ol": (m_drop("hl"), "fewbit", _ALL),
    "drop vl.oh": (m_drop("lh"), "fewbit", _ALL),
    "vl.ol added": (m_add_ll, "fewbit", _ALL),
    "k-halves swapped (v)": (m_swap_khalves, "fewbit", _ALL),
    "lo plane of the next row (O)": (m_lo_neighbour_row, "fewbit", _ALL),
    "k tail read from the next row": (m_tail_from_next_row, "tail", lambda case: case.shape.c % 16 != 0),
    "row N read by the last column": (m_row_past_n, "fewbit", _ALL),
    "floor(log2 mx) one too small at 2^k": (m_shift_at_pow2(+1), "sublo", _ALL),
    "floor(log2 mx) one too large at 2^k": (m_shift_at_pow2(-1), "sublo", _ALL),
    "row maximum over one k-half": (m_max_one_khalf, "tail", lambda case: case.shape.c > 8),
    "row factor of row r + 4": (m_row_factor_r4, "fewbit", lambda case: case.shape.B > 4),
    "O factor of the next column": (m_col_factor_neighbour, "fewbit", _ALL),
    "fifth group: a k-step missing": (m_fifth_missing_kstep, "fewbit", lambda case: case.fifth is not None and bool(case.fifth.any())),
    "hi truncated": (m_hi_truncated, "fewbit", _ALL),
}


def window(case, width=512):
    """A case cut to its first and last `width` entity rows (mutants are column-local up to a neighbour: the host test
    need not run each of them on 40 943 columns).  Keeps the guard row, and the fifth mask's entries."""
    s = case.shape
    if s.N <= 2 * width:
        return case
    keep = np.r_[0:width, s.N - width:s.N]
    sub = Shape(keep.size, s.c, s.B, 0, s.o_off, s.note)
    obuf = np.concatenate([case.obuf[:s.o_off], case.O[keep].ravel(), case.guard_row])
    return Case(case.name + "[window]", case.family, sub, case.v, obuf, None if case.valid is None else case.valid[:, keep],
                None if case.fifth is None else case.fifth[keep])
