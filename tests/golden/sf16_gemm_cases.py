"""A numpy model of the split-fp16 GEMM (rtk_gemm_sf16_splitk, csrc/rtk_gemm_sf16.hip) and operands on which the model
is EXACT, so that the kernel has to return it bit for bit whatever its summation order.  numpy only.  The split, the
planes, the product unit and the cap come from split_cases.py, gamma from exact_cases.py.

    e      = operand_shift(bound)   from the bound's bit pattern: 14 - (biased exponent - 127), at most E_MAX = 100; 0 for
                                    a zero, subnormal, inf or nan bound.  (rtk_pack_shift differs: it scales a subnormal.)
    hi, lo = fp16(x 2^e), fp16(x 2^e - hi)
    acc    = ah.bh + ah.bl + al.bh                                  (float64 here; exact fp16 products, fp32 adds there)
    C      = fp32(fp32(acc u1) u2),  u1 = 2^clamp(s, -126, 127), u2 = 2^(s - clamp(s)),  s = -(ea + eb)
             -- one factor whenever 2^s is an fp32 normal; otherwise two of the same sign, so that neither step over- or
             underflows unless the result does.
    split-K: k_chunk = ceil(ceil(K / splits) / 32) 32; chunk z covers [z k_chunk, min(K, (z + 1) k_chunk)) (empty: a
             zero slab); every slab is unscaled on its own and the slabs are added in chunk order in fp32.

Exactness (assert_exact, as split_cases.assert_exact): every product of a case is a multiple of a power of two g and,
per output, the absolute values of the 3 K products -- over the WHOLE K, so that the slab adds cannot round either --
sum to at most 2^23 g.  Outputs whose unit or abs-sum leaves fp32's normal range are masked (Case.valid).  Densities
are lowered until the cap holds; the cap is never raised.

Families -- every operand has ONE power-of-two unit, taken from its global bound:
    fewbit    split_cases' fewbit rows (both lo planes populated, signs mixed, zeros), bound = 3 x the true maximum
    hionly    +-(1..7) 2^11, lo = 0, for long K: addressing, tails, chunk boundaries and the slab order
    tail      one element per row equal to the bound, at k = K - 1, k = 0 or in the last second k-half, the rest a
              quarter as large
    bound:*   the bound against the true maximum: ratios 1, 3 and 2^10 over rows with 24-bit elements; bounds of exactly
              2^k, (2 - 2^-23) 2^k, 2^k (1 + 2^-23) met by an element; an all-zero operand with bound 0; -0.0; a
              subnormal bound over a subnormal operand, an inf and a nan bound over an operand inside fp16's range (scale
              1); a bound of 2^120 met by an element (below the shift's old lower clamp)
    scale:a:b bounds 2^a and 2^b over SCALE_EXPS^2, the pairs whose outputs are all fp32 normals
    scalepos:a:b  the same with positive elements (4..7) 2^11 next to the bound, on POS_SHAPE (K = 97): an accumulator of
              2^32 and more, which times 2^-ea alone overflows at a bound of 2^110 against one of 2^-60
    sublo15, sublo   elements at 2^-15 .. 2^-26 of a bound of exactly 2^k facing maximal elements
"""
import zlib
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

import split_cases as sc
from exact_cases import gamma
from split_cases import CAP, Planes, product_unit, split

F32, F16, F64 = np.float32, np.float16, np.float64
BK = 32
E_MAX = 100                                   # operand_scale's upper clamp; below, the exponent field ends at 14 - 127
SCALE_EXPS = (-120, -60, -40, 0, 40, 60, 110, 125)      # 125: a bound that the shift's lower clamp of -100 used to miss
LAYOUTS = ((1, 1), (1, 0), (0, 1), (0, 0))              # (a_kmajor, b_kmajor)
NAN_BITS, INF_BITS = 0x7FC00123, 0xFF800000             # what a K-major operand's padding holds besides finite garbage
MGARBAGE = F32(-1.5e30)                                  # an M-major operand's padding and its row K


# ---- the model ----------------------------------------------------------------------------------------------------
def operand_shift(bound):
    """operand_scale: the shift of a bound (array in, int64 array out)"""
    bits = np.ascontiguousarray(bound, dtype=F32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    ex = (bits >> np.uint32(23)).astype(np.int64)
    return np.where((ex == 0) | (ex == 255), 0, np.minimum(14 - (ex - 127), E_MAX)).astype(np.int64)


def planes(A, B, ba, bb, shift=operand_shift, round_hi=None):
    """split_cases.Planes of the logical (M, K) and (N, K) operands under their global bounds"""
    ah, al, ea = split(A, bound=ba, shift=shift, round_hi=round_hi)
    bh, bl, eb = split(B, bound=bb, shift=shift, round_hi=round_hi)
    return Planes(ah.astype(F64), al.astype(F64), ea, bh.astype(F64), bl.astype(F64), eb)


def chunks(K, splits):
    if splits == 1:
        return [(0, K)]
    kc = -(-(-(-K // splits)) // BK) * BK
    return [(min(K, z * kc), min(K, (z + 1) * kc)) for z in range(splits)]


def factors(ea, eb):
    """(u1, u2) of the epilogue, fp32"""
    s = -(int(ea) + int(eb))
    s1 = max(-126, min(127, s))
    return F32(np.ldexp(1.0, s1)), F32(np.ldexp(1.0, s - s1))


def merged_factor(ea, eb):
    """a mutant's single factor, built from the exponent field as the kernel builds its factors"""
    return np.array([((127 - int(ea) - int(eb)) << 23) & 0xFFFFFFFF], dtype=np.uint32).view(F32)[0]


def chain(P, k0, k1):
    sl = slice(k0, k1)
    return P.vh[:, sl] @ (P.oh[:, sl] + P.ol[:, sl]).T + P.vl[:, sl] @ P.oh[:, sl].T


def unscale32(acc, u):
    """the epilogue on an accumulator (float64 holding an fp32 value in the exact cases)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = acc.astype(F32)
        for f in u:
            y = y * f
    return y


def reduce32(slabs):
    with np.errstate(over="ignore", invalid="ignore"):
        C = slabs[0]
        for s in slabs[1:]:
            C = C + s
    return C


Model = namedtuple("Model", "C C64 T acc Tacc ea eb")


def gemm_model(P, K, splits=1, cks=None, u=None, skip_slab=None):
    """C: what the kernel returns (fp32); C64 / T: the same sum and its abs-sum in float64, unscaled (the real layer's
    reference); acc / Tacc: in accumulator units over the whole K.  cks, u, skip_slab exist for the mutants."""
    ea, eb = int(P.shv[0]), int(P.sho[0])
    cks = cks or chunks(K, splits)
    u = u or factors(ea, eb)
    accs = [chain(P, k0, k1) for k0, k1 in cks]
    C = reduce32([unscale32(a, u) for z, a in enumerate(accs) if z != skip_slab])
    acc = chain(P, 0, P.vh.shape[1])
    Tacc = np.abs(P.vh) @ (np.abs(P.oh) + np.abs(P.ol)).T + np.abs(P.vl) @ np.abs(P.oh).T
    return Model(C, np.ldexp(acc, -(ea + eb)), np.ldexp(Tacc, -(ea + eb)), acc, Tacc, ea, eb)


def real_bound(m, K, splits):
    """|C - C64| <= gamma(3 K_chunk + splits) T: 3 K_chunk terms in a slab's chain, splits - 1 slab adds, the unscaling
    (powers of two) exact for a normal result"""
    kc = max(k1 - k0 for k0, k1 in chunks(K, splits))
    return gamma(3.0 * kc + splits) * m.T


# ---- shapes ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shape:
    M: int
    N: int
    K: int
    splits: int = 1
    mode: str = "vec"       # K-major storage: vec (16-byte base, ld % 4 == 0), off (base one float on), odd (ld % 4 != 0)
    ldc_pad: int = 0
    c_off: int = 0
    note: str = ""

    @property
    def id(self):
        return (f"M{self.M}-N{self.N}-K{self.K}-s{self.splits}-{self.mode}" + (f"-ldc{self.ldc_pad}" if self.ldc_pad else "")
                + (f"-coff{self.c_off}" if self.c_off else ""))

    @property
    def tiles(self):
        return -(-self.M // 128) * -(-self.N // 128) * self.splits

    def pad_off(self, kmajor, length):
        """(pad, off) of an operand whose rows hold `length` floats"""
        if not kmajor:
            return 3, 0
        if self.mode == "vec":
            return (-length) % 4 + 4, 0
        if self.mode == "off":
            return (-length) % 4 + 4, 1
        return (-length) % 4 + 1, 0


def _s(M, N, K, splits=1, mode="vec", ldc_pad=0, c_off=0, note=""):
    return Shape(M, N, K, splits, mode, ldc_pad, c_off, note)


K_SWEEP = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 161)
MN_SWEEP = ((1, 257), (31, 129), (32, 128), (33, 127), (64, 65), (65, 64), (127, 33), (128, 32), (129, 31), (257, 1))
SHAPES = (
    [_s(33, 31, K, note="K sweep: every fragment edge, one tile and two, odd and even tile counts") for K in K_SWEEP]
    + [_s(33, 31, K, mode="off") for K in (7, 33, 97)] + [_s(33, 31, K, mode="odd") for K in (9, 65, 161)]
    + [_s(M, N, 33, mode=("vec", "off", "odd")[i % 3], note="M, N sweep") for i, (M, N) in enumerate(MN_SWEEP)]
    + [
        _s(257, 129, 40, note="6 tiles"),
        _s(129, 129, 64, 2, note="8 tiles, equal chunks"),
        _s(257, 257, 17, note="9 tiles"),
        _s(2049, 1, 9, note="17 tiles"),
        _s(257, 129, 100, 3, note="18 tiles; a last chunk that starts past K"),
        _s(33, 31, 161, 2, note="ragged last chunk; M N 4 % 256 != 0"),
        _s(33, 31, 97, 3, mode="odd", note="ragged, the third chunk past K"),
        _s(33, 31, 65, 4, mode="off", note="a last chunk that starts past K"),
        _s(33, 31, 33, 7, note="splits > K / 32"),
        _s(70, 36, 515, 4, note="four chunks of 160, the last ragged"),
        _s(33, 31, 97, 1, ldc_pad=5, c_off=1, note="ldc > N, C off its alignment"),
        _s(130, 70, 97, 1, ldc_pad=2, note="the control shape"),
    ]
)
SHAPE_IDS = [s.id for s in SHAPES]
LONG = _s(130, 70, 20011, 7, note="the long dv-like case (hionly)")
SMALL = _s(33, 31, 33)                       # where the bound and scale families run (and SMALL_SPLIT)
SMALL_SPLIT = _s(33, 31, 65, 2, mode="odd")
CONTROL = SHAPES[-1]

BOUND_VARIANTS = ("ratio1", "ratio3", "ratio1024", "pow2", "below_pow2", "above_pow2", "zero", "negzero", "subnormal",
                  "inf", "nan", "huge")
FAMILIES_ALL_SHAPES = ("fewbit", "hionly", "tail", "sublo15", "sublo")


POS_SHAPE = _s(33, 31, 97)


def pos_families():
    return [f"scalepos:{a}:{b}" for a in SCALE_EXPS for b in SCALE_EXPS]


def small_families():
    return [f"bound:{v}:{side}" for v in BOUND_VARIANTS for side in "AB"] + [f"scale:{a}:{b}" for a in SCALE_EXPS for b in SCALE_EXPS]


# ---- cases ----------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    family: str
    shape: Shape
    A: np.ndarray           # (M, K) fp32, logical
    B: np.ndarray           # (N, K)
    ba: np.float32
    bb: np.float32
    P: object = None
    model: object = None
    g: float = None
    valid: np.ndarray = None


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _units(y, E):
    """accumulator units -> fp32: y 2^(E - 14), exact"""
    return sc._to_rows(y, np.full(y.shape[0], E))


def tail_positions(K):
    """k = K - 1, k = 0 and the last k of a second k-half (k % 16 >= 8), where there is one"""
    pos = [K - 1, 0]
    k2 = max((k for k in range(max(0, K - 17), K) if k % 16 >= 8), default=None)
    if k2 is not None:
        pos.append(k2)
    return pos


def _hionly_rows(rng, R, K, density):
    y = rng.integers(1, 8, size=(R, K)) * 2048.0 * rng.choice([-1.0, 1.0], size=(R, K)) * (rng.random((R, K)) < density)
    y[np.arange(R), rng.integers(0, K, size=R)] = 7 * 2048.0
    return y


def _operands(family, shape, rng, density):
    """(A, B, ba, bb) of a family; the bound variants and scale pairs change one or both operands of a fewbit pair"""
    M, N, K = shape.M, shape.N, shape.K
    kind, *arg = family.split(":")
    EA, EB = 3, -2                                                    # different: exchanged scales must show
    if kind in ("fewbit", "scale"):
        yA, yB = sc._fewbit_rows(rng, M, K, density), sc._fewbit_rows(rng, N, K, density)
        if K == 1:      # split_cases gives a row's only element to its maximum, 16384 + 2 b: put the other kind there too
            for y in (yA, yB):
                odd = np.arange(1, y.shape[0], 2)
                y[odd, 0] = (12288.0 + odd % 7 - 3) * np.where(odd % 4 == 1, 1.0, -1.0)
        if kind == "scale":
            EA, EB = int(arg[0]), int(arg[1])                         # bound 2^E over elements below 2^(E - 1) 1.001
            return _units(yA, EA - 1), _units(yB, EB - 1), F32(2.0) ** F32(EA), F32(2.0) ** F32(EB)
        A, B = _units(yA, EA), _units(yB, EB)
        return A, B, F32(3 * np.abs(A).max()), F32(3 * np.abs(B).max())
    if kind == "scalepos":                   # no cancellation: |acc| >= 16 K 2^22 >= 2^32 from K = 64 on
        EA, EB = int(arg[0]), int(arg[1])
        yA, yB = rng.integers(4, 8, size=(M, K)) * 2048.0, rng.integers(4, 8, size=(N, K)) * 2048.0
        return _units(yA, EA), _units(yB, EB), F32(2.0) ** F32(EA), F32(2.0) ** F32(EB)
    if kind == "hionly":
        A, B = _units(_hionly_rows(rng, M, K, density), EA), _units(_hionly_rows(rng, N, K, density), EB)
        return A, B, F32(3 * np.abs(A).max()), F32(3 * np.abs(B).max())
    if kind == "tail":
        pos = tail_positions(K)
        out = []
        for R in (M, N):
            y = sc._fewbit_rows(rng, R, K, density, 0.25)
            y[np.arange(R), np.asarray(pos)[np.arange(R) % len(pos)]] = rng.choice([-1.0, 1.0], size=R) * 16390.0
            out.append(y)
        A, B = _units(out[0], EA), _units(out[1], EB)
        return A, B, F32(np.abs(A).max()), F32(np.abs(B).max())
    if kind in ("sublo15", "sublo"):
        ks = (15, 16) if kind == "sublo15" else tuple(range(17, 27))
        A, B = _units(_sublo(rng, M, K, True, ks), EA), _units(_sublo(rng, N, K, False, ks), EB)
        return A, B, F32(np.abs(A).max()), F32(np.abs(B).max())       # exactly 2^EA, 2^EB
    assert kind == "bound"
    variant, side = arg
    other = _units(_coarse(rng, N if side == "A" else M, K, density), EB)
    R = M if side == "A" else N
    if variant.startswith("ratio"):
        ks = tuple(range(17, 27))                   # 24-bit elements: what the shift leaves of them depends on the bound
        X, other = _units(_sublo(rng, R, K, True, ks), EA), _units(_sublo(rng, other.shape[0], K, False, ks), EB)
        bx, bo = F32(float(variant[5:]) * np.abs(X).max()), F32(np.abs(other).max())
        return (X, other, bx, bo) if side == "A" else (other, X, bo, bx)
    elif variant in ("pow2", "below_pow2", "above_pow2", "huge"):
        top = {"pow2": 1.0, "below_pow2": 2.0 - 2.0 ** -23, "above_pow2": 1.0 + 2.0 ** -23, "huge": 1.0}[variant] * 16384.0
        y = _coarse(rng, R, K, density) / 2
        y[:, 0] = 0.0
        y[R // 2, 0] = -top                       # meets the bound; faces a zero (with its lo = -+2^-9 no cap could hold)
        other[:, 0] = 0.0
        X = _units(y, 120 if variant == "huge" else EA)
        bx = F32(np.abs(X).max())
    elif variant in ("zero", "negzero"):
        X = np.full((R, K), 0.0 if variant == "zero" else -0.0, dtype=F32)
        bx = F32(0.0)
    elif variant == "subnormal":
        X = (rng.integers(-7, 8, size=(R, K)) * 2.0 ** -149).astype(F32)
        X[0, 0] = F32(2.0 ** -127)
        bx = F32(2.0 ** -127)
    else:                                          # inf, nan: scale 1, the operand inside fp16's range as it stands
        X = _units(_coarse(rng, R, K, density), 14 - 3)
        bx = F32(np.inf) if variant == "inf" else F32(np.nan)
    bo = F32(3 * np.abs(other).max())
    return (X, other, bx, bo) if side == "A" else (other, X, bo, bx)


def _coarse(rng, R, K, density):
    """sparse coarse values with lo = 0 (also after a halving or a shift by three bits)"""
    fill = np.array([8192.0, -8192.0, 4096.0, -4096.0, 6144.0, -6144.0, 12288.0, -12288.0])
    return fill[rng.integers(0, len(fill), size=(R, K))] * (rng.random((R, K)) < density)


def _sublo(rng, R, K, first, ks):
    """split_cases' sublo rows: the maximum 2^14 and one tiny element per row, at opposite ends of the row for the two
    operands (K = 1: the maximum alone)"""
    if K == 1:
        return np.full((R, 1), 16384.0) * rng.choice([-1.0, 1.0], size=(R, 1))
    return sc._sublo_rows(rng, R, K, K - 1 if first else 0, 0 if first else K - 1, ks)


def make_case(shape, family):
    """The exact case of a family on a shape, or None for a scale pair whose outputs are not all fp32 normals."""
    name = f"{family}/{shape.id}"
    density = 0.9
    for _ in range(40):
        A, B, ba, bb = _operands(family, shape, _rng(name), density)
        P = planes(A, B, ba, bb)
        m = gemm_model(P, shape.K, shape.splits)
        g = product_unit(P)
        if m.Tacc.max() / g <= CAP:
            unit = np.ldexp(g, -(m.ea + m.eb))
            valid = np.full(m.C.shape, bool(unit >= 2.0 ** -126)) & (m.T < 2.0 ** 127)
            if family.startswith("scale") and not (valid.all() and m.T.min() >= 2.0 ** -126):
                return None
            return Case(name, family, shape, A, B, ba, bb, P, m, g, valid)
        density *= 0.9
    raise AssertionError(f"{name}: no density meets the cap")


def assert_exact(case):
    """The criterion of an exact case -> headroom max T / g."""
    m, P, g, ok = case.model, case.P, case.g, case.valid
    kind = case.family.split(":")[0]
    assert np.isfinite(m.acc).all(), case.name
    head = float(m.Tacc.max() / g)
    assert head <= CAP, f"{case.name}: max T / g = 2^{np.log2(head):.2f} > 2^23"
    assert np.array_equal(m.acc / g, np.rint(m.acc / g)), case.name
    C = m.C.astype(F64)
    assert np.isfinite(C[ok]).all() and np.array_equal(C[ok], m.C64[ok]), f"{case.name}: the model is not the exact sum"
    assert (np.abs(C[ok])[C[ok] != 0] >= 2.0 ** -126).all(), case.name
    # C + al.bl is the float64 product of the fp32 operands wherever hi + lo holds the scaled operand
    ya, yb = np.ldexp(case.A.astype(F64), m.ea), np.ldexp(case.B.astype(F64), m.eb)
    da, db = ya - P.vh - P.vl, yb - P.oh - P.ol
    if kind in ("fewbit", "hionly", "tail", "sublo15") or (kind == "scale" and max(m.ea, m.eb) < E_MAX):
        assert not da.any() and not db.any(), f"{case.name}: hi + lo does not hold the operand"
    if not da.any() and not db.any():
        z64 = case.A.astype(F64) @ case.B.astype(F64).T
        assert np.array_equal((m.C64 + np.ldexp(P.vl @ P.ol.T, -(m.ea + m.eb)))[ok], z64[ok]), f"{case.name}: C + al.bl != A B^T"
    return head


def real_case(shape, mag_a, mag_b):
    """normals times exp(uniform(-6, 0)) per element, at the magnitudes of test_gemm_split_fp16_against_float64"""
    rng = _rng(f"real/{shape.id}/{mag_a}/{mag_b}")
    A = (rng.standard_normal((shape.M, shape.K)) * np.exp(rng.uniform(-6, 0, (shape.M, shape.K))) * mag_a).astype(F32)
    B = (rng.standard_normal((shape.N, shape.K)) * np.exp(rng.uniform(-6, 0, (shape.N, shape.K))) * mag_b).astype(F32)
    return Case(f"real/{shape.id}/{mag_a:g}x{mag_b:g}", "real", shape, A, B, F32(np.abs(A).max()), F32(np.abs(B).max()))


# ---- storage (shared by the device test and the tail mutants) --------------------------------------------------------
def lay_out(X, kmajor, pad, off):
    """Flat fp32 storage of the logical (rows, K) operand X -> (flat, offset of the base, ld).  K-major: rows of K + pad
    floats, the padding cycling through finite garbage, nan and inf bit patterns (the kernel may read it and must
    select it away).  M-major: K + 1 rows of rows + pad floats, the padding and row K huge and finite (never read)."""
    rows, K = X.shape
    if kmajor:
        st = np.empty((rows, K + pad), dtype=F32)
        fill = np.array([0x7149F2CA, NAN_BITS, INF_BITS, 0x7F800000, 0xFFC00000, 0xF149F2CA], dtype=np.uint32).view(F32)
        st[:] = fill[(np.arange(rows)[:, None] + np.arange(K + pad)[None, :]) % len(fill)]
        st[:, :K] = X
    else:
        st = np.full((K + 1, rows + pad), MGARBAGE, dtype=F32)
        st[:K, :rows] = X.T
    front = np.full(off, MGARBAGE, dtype=F32)
    return np.concatenate([front, st.reshape(-1), np.full(16, MGARBAGE, dtype=F32)]), off, st.shape[1]


# ---- mutants: each returns a wrong C (fp32) for a case -----------------------------------------------------------------
def _mut(case, P=None, **kw):
    return gemm_model(P or case.P, case.shape.K, case.shape.splits, **kw).C


def m_drop(term):
    def f(case):
        P = case.P
        z = np.zeros_like
        Q = {"hh": None, "hl": P._replace(ol=z(P.ol)), "lh": P._replace(vl=z(P.vl))}[term]
        if Q is not None:
            return _mut(case, Q)
        full = [chain(P, k0, k1) - P.vh[:, k0:k1] @ P.oh[:, k0:k1].T for k0, k1 in chunks(case.shape.K, case.shape.splits)]
        return reduce32([unscale32(a, factors(case.model.ea, case.model.eb)) for a in full])
    return f


def m_add_ll(case):
    P = case.P
    accs = [chain(P, k0, k1) + P.vl[:, k0:k1] @ P.ol[:, k0:k1].T for k0, k1 in chunks(case.shape.K, case.shape.splits)]
    return reduce32([unscale32(a, factors(case.model.ea, case.model.eb)) for a in accs])


def m_hi_truncated(case):
    return _mut(case, planes(case.A, case.B, case.ba, case.bb, round_hi=sc._truncate_f16))


def m_shift_at_pow2(delta):
    def shift(b):
        m, _ = np.frexp(np.asarray(b, dtype=F32))
        return operand_shift(b) + delta * (m == 0.5)
    return lambda case: _mut(case, planes(case.A, case.B, case.ba, case.bb, shift=shift))


def m_shift_from_true_max(case):
    return _mut(case, planes(case.A, case.B, F32(np.abs(case.A).max()), F32(np.abs(case.B).max())))


def m_scales_exchanged(case):
    with np.errstate(over="ignore", invalid="ignore"):
        return _mut(case, planes(case.A, case.B, case.bb, case.ba))


def m_swap_khalves(case):
    P, K = case.P, case.shape.K
    K16 = -(-K // 16) * 16
    sw = lambda x: sc._pad(x, K16).reshape(x.shape[0], -1, 2, 8)[:, :, ::-1, :].reshape(x.shape[0], K16)
    Q = Planes(sw(P.vh), sw(P.vl), P.shv, sc._pad(P.oh, K16), sc._pad(P.ol, K16), P.sho)
    return _mut(case, Q, cks=[(k0, K16 if k0 < k1 == K else k1) for k0, k1 in chunks(K, case.shape.splits)])


def m_lo_next_row(case):
    return _mut(case, case.P._replace(ol=np.roll(case.P.ol, -1, axis=0)))


def _last_chunk_widened(case, widen):
    """both operands' K tail filled by `widen` up to the end of the last k-tile, and the chunk that ends at K with it"""
    K = case.shape.K
    K32 = -(-K // BK) * BK
    P = planes(widen(case.A, K32), widen(case.B, K32), case.ba, case.bb)
    return _mut(case, P, cks=[(k0, K32 if k1 == K and k0 < K else k1) for k0, k1 in chunks(K, case.shape.splits)])


def m_kmajor_tail(case):
    """dense K-major rows, the tail not zeroed: it reads on into the next row (behind the last row: nothing, zeros)"""
    def widen(X, K32):
        rows, K = X.shape
        flat = np.concatenate([X.ravel(), np.zeros(K32, dtype=F32)])
        return flat[np.arange(rows)[:, None] * K + np.arange(K32)[None, :]]
    return _last_chunk_widened(case, widen)


def m_mmajor_tail(case):
    """M-major, the tail not zeroed: the clamped last k is counted again"""
    return _last_chunk_widened(case, lambda X, K32: np.concatenate([X, np.repeat(X[:, -1:], K32 - X.shape[1], axis=1)], axis=1))


def m_chunk_boundary(delta):
    def f(case):
        cks = chunks(case.shape.K, case.shape.splits)
        return _mut(case, cks=[(k0 + delta if 0 < k0 < k1 else k0, k1) for k0, k1 in cks])
    return f


def m_slab_left_out(case):
    return _mut(case, skip_slab=1)


def m_unscale_merged(case):
    return _mut(case, u=(merged_factor(case.model.ea, case.model.eb),))


def _two_chunks(case):
    cks = chunks(case.shape.K, case.shape.splits)
    return len(cks) > 1 and cks[1][1] > cks[1][0]


_ALL = lambda case: True
_TAIL = lambda case: case.shape.K % BK != 0
# name -> (function, the family whose cases must catch it, which cases it applies to)
MUTANTS = {
    "drop ah.bh": (m_drop("hh"), "fewbit", _ALL),
    "drop ah.bl": (m_drop("hl"), "fewbit", _ALL),
    "drop al.bh": (m_drop("lh"), "fewbit", _ALL),
    "al.bl added": (m_add_ll, "fewbit", _ALL),
    "hi truncated": (m_hi_truncated, "fewbit", _ALL),
    "shift one too large at a bound of 2^k": (m_shift_at_pow2(+1), "sublo", lambda case: case.shape.K > 1),
    "shift one too small at a bound of 2^k": (m_shift_at_pow2(-1), "sublo", lambda case: case.shape.K > 1),
    "shift from the true maximum": (m_shift_from_true_max, "bound:ratio1024:A", _ALL),
    "operand scales exchanged": (m_scales_exchanged, "fewbit", _ALL),
    "k-halves swapped (A)": (m_swap_khalves, "fewbit", _ALL),
    "lo plane of the next row (B)": (m_lo_next_row, "fewbit", lambda case: case.shape.N > 1),
    "K-major tail not zeroed": (m_kmajor_tail, "hionly", lambda case: _TAIL(case) and min(case.shape.M, case.shape.N) > 1),
    "M-major tail not zeroed": (m_mmajor_tail, "hionly", _TAIL),
    "chunk boundary overlaps by one k": (m_chunk_boundary(-1), "hionly", _two_chunks),
    "chunk boundary leaves a gap of one k": (m_chunk_boundary(+1), "hionly", _two_chunks),
    "slab 1 left out of the reduce": (m_slab_left_out, "hionly", _two_chunks),
    "unscale factors merged": (m_unscale_merged, "scale", lambda case: not -126 <= -(case.model.ea + case.model.eb) <= 127),
}
