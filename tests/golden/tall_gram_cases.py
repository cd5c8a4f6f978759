"""The float64 tall Gram product (``rtk_tall_gram_f64``, csrc/rtk_tall_gram.hip): cases, reference, bounds, a float64
emulation of the kernel's split, and the mutants that the bounds must catch.

The operation, as the header states it: ``C[i, j] = sum_{k < n} A[k, i] * B[k, j]`` (p x q, float64) for fp32 A (n x p)
and B (n x q) at row pitches lda >= p, ldb >= q, every product and every sum in float64.  An operand is described as
the ABI takes it: a flat fp32 buffer, an element offset and a pitch.

Two families:

  E  integer-valued fp32 entries, |x| <= 2^10.  A product is below 2^20 and a sum of n <= 2^13 of them below 2^33:
     every partial sum is an integer that float64 holds exactly, whatever the order.  The result must be BIT-EQUAL to
     the reference.
  G  full-mantissa entries (standard normal, rounded to fp32).  The reference is ``A.astype(f64).T @ B.astype(f64)`` and
     the bound per entry is  ``2 * 1.01 * n * u * (|A|^T |B|)[i, j]``,  u = 2^-53:  a product of two fp32 values has 48
     significant bits and is exact in float64; n float64 additions in ANY order lose at most n u (1 + O(n u)) of the sum
     of the absolute values (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; 1.01 covers the second
     order term for n u < 0.01); once for the kernel and once for the reference, whose order is BLAS's.

Layouts: ``contig`` (two matrices of their own, pitch = width: the 16-byte path where p % 4 == q % 4 == 0), ``gram``
(A and B the same matrix), ``halves`` (p == q: the column halves of one n x 2p matrix, pitch 2p), ``odd`` (views at odd
column offsets: A at column 1 of an n x (p + 4) matrix -- a pitch the 16-byte path would take, a base it cannot --, B at
column 3 of an n x (q + 5) matrix: the element path).

Host-only (numpy)."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -53
TILE, KC, MIN_ROWS, TARGET_WG, WS_MAX, PQ_MAX = 64, 32, 1024, 1024, 64 << 20, 1024     # csrc/rtk_tall_gram.hip

NS = (1, 3, 63, 1000, 4099, 2500)            # 2500: three ranges of 1024 rows, the last one 452 rows short of full
SHAPES = ((1, 1), (8, 8), (20, 12), (200, 200), (208, 64), (512, 512), (1024, 16))
FAMILIES = ("E", "G")
LAYOUTS = ("contig", "gram", "halves", "odd")

LABELS = frozenset({
    "vec", "scalar", "pitch_above_width", "base_misaligned", "pitch_not_mult4", "same_operand",
    "one_range", "several_ranges", "three_ranges_short_last", "last_range_under_a_chunk", "n_below_4", "row_tail",
    "one_tile", "several_tiles", "col_tail_16", "wave_without_columns", "p_ne_q", "full_tile",
})


def _cdiv(a, b):
    return -(-a // b)


def tiles(p, q):
    return _cdiv(p, TILE) * _cdiv(q, TILE)


def split(n, p, q):
    """``(len, ranges)``: the kernel's static cut of the rows (``tall_gram_split``)."""
    smax = max(1, min(TARGET_WG // tiles(p, q), WS_MAX // (p * q * 8)))
    length = _cdiv(max(_cdiv(n, smax), MIN_ROWS), KC) * KC
    return length, max(1, _cdiv(n, length))


def workspace_bytes(n, p, q):
    if n < 0 or not (1 <= p <= PQ_MAX and 1 <= q <= PQ_MAX):
        return 0
    return _cdiv(split(n, p, q)[1] * p * q * 8, 256) * 256


@dataclass(frozen=True)
class GramCase:
    name: str
    family: str
    n: int
    p: int
    q: int
    layout: str


def _cases():
    out = []
    for fam in FAMILIES:
        for n in NS:
            for p, q in SHAPES:
                out.append(GramCase(f"{fam}-n{n}-{p}x{q}-contig", fam, n, p, q, "contig"))
        for n in (63, 4099):
            for p, q in SHAPES:
                out.append(GramCase(f"{fam}-n{n}-{p}x{q}-odd", fam, n, p, q, "odd"))
        for n in (3, 1000, 2500):
            for p in (1, 8, 200, 512):
                out.append(GramCase(f"{fam}-n{n}-{p}x{p}-halves", fam, n, p, p, "halves"))
        for n, p in ((63, 20), (4099, 200)):
            out.append(GramCase(f"{fam}-n{n}-{p}x{p}-gram", fam, n, p, p, "gram"))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@dataclass(frozen=True)
class Operands:
    """What the ABI takes: flat fp32 buffers (``buf_a is buf_b`` when the operands share a matrix), element offsets,
    pitches."""
    buf_a: np.ndarray
    off_a: int
    lda: int
    buf_b: np.ndarray
    off_b: int
    ldb: int


def _fill(rng, family, shape):
    if family == "E":
        return rng.integers(-1024, 1025, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=8)
def operands(case):
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    n, p, q = case.n, case.p, case.q
    if case.layout == "contig":
        return Operands(_fill(rng, case.family, n * p), 0, p, _fill(rng, case.family, n * q), 0, q)
    if case.layout == "gram":
        buf = _fill(rng, case.family, n * p)
        return Operands(buf, 0, p, buf, 0, p)
    if case.layout == "halves":
        buf = _fill(rng, case.family, n * 2 * p)
        return Operands(buf, 0, 2 * p, buf, p, 2 * p)
    assert case.layout == "odd"
    return Operands(_fill(rng, case.family, n * (p + 4)), 1, p + 4, _fill(rng, case.family, n * (q + 5)), 3, q + 5)


def gather(buf, off, ld, n, cols):
    """The (n x cols) operand that the kernel reads from ``buf``: element (k, i) at ``off + k * ld + i``."""
    idx = off + np.arange(n, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]
    return buf[idx]


def matrices(case):
    op = operands(case)
    return gather(op.buf_a, op.off_a, op.lda, case.n, case.p), gather(op.buf_b, op.off_b, op.ldb, case.n, case.q)


def vector_path(case):
    """Whether the launcher takes the 16-byte loads (bases are 16-byte aligned when their element offset is 0 mod 4)."""
    op = operands(case)
    return (op.off_a % 4 == 0 and op.off_b % 4 == 0 and op.lda % 4 == 0 and op.ldb % 4 == 0
            and case.p % 4 == 0 and case.q % 4 == 0)


def features(case):
    op = operands(case)
    n, p, q = case.n, case.p, case.q
    length, ranges = split(n, p, q)
    f = {"vec" if vector_path(case) else "scalar"}
    if op.lda > p or op.ldb > q:
        f.add("pitch_above_width")
    if op.off_a % 4 or op.off_b % 4:
        f.add("base_misaligned")
    if op.lda % 4 or op.ldb % 4:
        f.add("pitch_not_mult4")
    if op.buf_a is op.buf_b and op.off_a == op.off_b:
        f.add("same_operand")
    f.add("one_range" if ranges == 1 else "several_ranges")
    last = n - (ranges - 1) * length
    if ranges >= 3 and last < length:
        f.add("three_ranges_short_last")
    if ranges > 1 and last < KC:
        f.add("last_range_under_a_chunk")
    if n < 4:
        f.add("n_below_4")
    if n % KC:
        f.add("row_tail")
    f.add("one_tile" if p <= TILE and q <= TILE else "several_tiles")
    if p % 16 or q % 16:
        f.add("col_tail_16")
    if 0 < p % TILE <= 32 or 0 < q % TILE <= 32:
        f.add("wave_without_columns")
    if p % TILE == 0 and q % TILE == 0:
        f.add("full_tile")
    if p != q:
        f.add("p_ne_q")
    return f


def reference(case):
    A, B = matrices(case)
    return A.astype(np.float64).T @ B.astype(np.float64)


def bound(case):
    """Per entry; zeros for family E (bit equality)."""
    if case.family == "E":
        return np.zeros((case.p, case.q))
    A, B = matrices(case)
    return 2 * 1.01 * case.n * U * (np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64))


def inside(case, C, ref=None, bnd=None):
    """``(ok, worst)``: whether C (p x q float64) meets the case's bound, and max error / bound (family E: the number of
    entries that differ)."""
    ref = reference(case) if ref is None else ref
    if C.shape != ref.shape:
        return False, float("inf")
    if case.family == "E":
        bad = int((C != ref).sum()) + int((~np.isfinite(C)).sum())
        return bad == 0, float(bad)
    bnd = bound(case) if bnd is None else bnd
    err = np.abs(C - ref)
    if not np.isfinite(C).all():
        return False, float("inf")
    ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
    return bool((err <= bnd).all()), float(ratio.max())


MUTANTS = ("f32_accumulate", "drop_last_row", "drop_col_tail", "pitch_as_p", "lose_partial", "transpose_c")


def emulate(case, mutant=None):
    """The kernel's split in float64 with ANOTHER order inside the ranges (numpy's product, rows descending): range
    partials, added in range order.  ``mutant``: one of MUTANTS, the defect that it stands for:
      f32_accumulate  the sums (and products) in fp32;
      drop_last_row   row n - 1 is never read;
      drop_col_tail   the last p % 16 columns of A contribute nothing (those rows of C stay zero);
      pitch_as_p      A is read at pitch p instead of lda;
      lose_partial    the second range's partial is not added (the first one's when there is one range);
      transpose_c     the result is written as its transpose into the p x q buffer."""
    assert mutant is None or mutant in MUTANTS
    op = operands(case)
    n, p, q = case.n, case.p, case.q
    A = gather(op.buf_a, op.off_a, p if mutant == "pitch_as_p" else op.lda, n, p)
    B = gather(op.buf_b, op.off_b, op.ldb, n, q)
    if mutant == "drop_last_row":
        A, B, n = A[:-1], B[:-1], n - 1
    dt = np.float32 if mutant == "f32_accumulate" else np.float64
    length, ranges = split(case.n, p, q)
    C = np.zeros((p, q), dtype=dt)
    for s in range(ranges):
        if mutant == "lose_partial" and s == min(1, ranges - 1):
            continue
        a, b = A[s * length:min(n, (s + 1) * length)][::-1], B[s * length:min(n, (s + 1) * length)][::-1]
        C = C + a.astype(dt).T @ b.astype(dt)
    C = C.astype(np.float64)
    if mutant == "drop_col_tail" and p % 16:
        C[p - p % 16:] = 0.0
    if mutant == "transpose_c":
        C = np.ascontiguousarray(C.T).reshape(p, q)
    return C
