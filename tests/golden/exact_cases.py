"""Operands for which fp32 cannot round, their float64 references and the case lists of the bit-exact tests.

The exact-fp32 GEMM (``rtk_gemm_f32*``) and the stage-1 backward (``rtk_query_vectors_bwd_f32``) do nothing but
fp32 fma chains and plain fp32 adds.  If every operand is an integer-valued fp32 and, for every output element,
the sum of the absolute values of all of its terms is below 2^24, then every product, every partial sum in any
order, every split-K slab and every scatter partial is an exactly representable integer: the kernel has to return
the float64 result bit for bit, whatever its summation order.  Two regimes:

  small   every operand in {-2..2} (thinned where the sums are long): coverage and indexing;
  wide    one operand holds odd integers of exactly 12 (or 20) significant bits, the others are sparse in
          {-1, 0, 1}: an fp16 / bf16 / tf32 shortcut on the wide operand breaks the equality.

The generators compute the abs-sum matrices in float64 and assert ``max < 2**24`` before anything is returned.
A smaller real-valued layer ("real": normals times exp(U(-6, 0)); "real_pow2": that times per-row powers of two
over 2^-20 .. 2^20) is checked against the derived bound ``gamma_n * sum|a||b|``, gamma_n = n u / (1 - n u),
u = 2^-24.

Host-only (numpy); ``tests/test_exact_cases_host.py`` proves the method on every case without a GPU, the GPU
files parametrize over the same lists.
"""
import zlib
from dataclasses import dataclass

import numpy as np

LIMIT = float(2 ** 24)
U = 2.0 ** -24
GARBAGE = 3.0          # what lies past a K tail or in row padding: a kernel that reads it changes the result
EXACT = ("small", "wide12", "wide20")


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def _seed(name):
    return zlib.crc32(name.encode())


def wide_ints(rng, shape, bits):
    """Odd integers with exactly `bits` significant bits and a random sign (fp32-exact for bits <= 24)."""
    v = rng.integers(2 ** (bits - 1), 2 ** bits, size=shape, dtype=np.int64) | 1
    return (v * rng.choice([-1, 1], size=shape)).astype(np.float32)


def small_ints(rng, shape, density=1.0):
    v = rng.integers(-2, 3, size=shape).astype(np.float32)
    if density < 1.0:
        v *= rng.random(shape) < density
    return v


def signs(rng, shape, density):
    return (rng.choice([-1.0, 1.0], size=shape) * (rng.random(shape) < density)).astype(np.float32)


def real_values(rng, shape, pow2_rows=False):
    v = rng.standard_normal(shape) * np.exp(rng.uniform(-6, 0, shape))
    if pow2_rows:
        v = v * 2.0 ** rng.integers(-20, 21, size=(shape[0],) + (1,) * (len(shape) - 1))
    return v.astype(np.float32)


def round_mantissa(x, bits):
    """x rounded (to nearest, ties to even) to `bits` significant bits: what a narrower format would keep."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.rint(m * 2.0 ** bits) / 2.0 ** bits, e).astype(np.float32)


# ---------------------------------------------------------------------------------------------- GEMM ------
@dataclass(frozen=True)
class GemmCase:
    """C (M x N) = A (M x K) . B (N x K)^T through one entry point of the C ABI.

    ak / bk: operand stored K-major (row = m, n) or M-major (row = k).  a_pad / b_pad: extra elements per stored
    row (the leading dimension is the row length plus the pad; a pad that is not a multiple of 4 takes the scalar
    load path), filled with GARBAGE.  a_off / b_off / c_off: the base pointer is moved by that many floats off a
    16-byte boundary.  ldc_pad: ldc - N.  splits: 0 = rtk_gemm_f32 (or rtk_score_f32 with entry="score"),
    >= 1 = rtk_gemm_f32_splitk."""
    name: str
    M: int
    N: int
    K: int
    ak: int = 1
    bk: int = 1
    regime: str = "small"
    wide: str = "A"
    a_pad: int = 0
    b_pad: int = 0
    a_off: int = 0
    b_off: int = 0
    c_off: int = 0
    ldc_pad: int = 0
    splits: int = 0
    entry: str = "gemm"

    @property
    def exact(self):
        return self.regime in EXACT

    @property
    def k_chunk(self):
        """K of one split-K chunk (the kernel's rule: ceil(K / splits) rounded up to the k-tile of 16)."""
        if self.splits <= 1:
            return self.K
        return -(-(-(-self.K // self.splits)) // 16) * 16


def gemm_operands(case, extra_k=0):
    """(A, B): fp32, logical shapes (M, K + extra_k) and (N, K + extra_k).  Columns past K hold GARBAGE (what a
    kernel that reads its K tail too far would meet).  For the exact regimes the 2^24 condition is asserted."""
    rng = np.random.default_rng(_seed(case.name))
    M, N, K = case.M, case.N, case.K
    if case.regime == "small":
        A, B = small_ints(rng, (M, K)), small_ints(rng, (N, K))
        A[:, K - 1][A[:, K - 1] == 0] = 1          # the last k-term is visible in every element
        B[:, K - 1][B[:, K - 1] == 0] = -1
    elif case.regime in ("wide12", "wide20"):
        bits = int(case.regime[4:])
        nnz = min(K, (2 ** 24 - 1) // (2 ** bits - 1))     # non-zeros per row of the sign operand: nnz * max|wide| < 2^24
        rows_w, rows_s = (M, N) if case.wide == "A" else (N, M)
        W = wide_ints(rng, (rows_w, K), bits)
        Sg = np.zeros((rows_s, K), dtype=np.float32)
        for i in range(rows_s):
            pos = rng.choice(K - 1, size=nnz - 1, replace=False) if nnz > 1 else np.zeros(0, dtype=np.int64)
            Sg[i, pos] = rng.choice([-1.0, 1.0], size=nnz - 1)
            Sg[i, K - 1] = 1.0 if i % 2 == 0 else -1.0     # the last k-term is visible in every element
        A, B = (W, Sg) if case.wide == "A" else (Sg, W)
    elif case.regime in ("real", "real_pow2"):
        A = real_values(rng, (M, K), pow2_rows=case.regime == "real_pow2")
        B = real_values(rng, (N, K))
    else:
        raise ValueError(case.regime)
    if case.exact:
        worst = float((np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T).max())
        assert worst < LIMIT, f"{case.name}: abs-sum {worst} >= 2^24 -- reshape the case"
    if extra_k:
        A = np.concatenate([A, np.full((M, extra_k), GARBAGE, np.float32)], axis=1)
        B = np.concatenate([B, np.full((N, extra_k), GARBAGE, np.float32)], axis=1)
    return A, B


def gemm_ref(A, B):
    return A.astype(np.float64) @ B.astype(np.float64).T


def gemm_bound(case, A, B):
    """gamma_n * sum_k |a||b| with n = the chunk's K + splits (one rounding per fma, one per slab add)."""
    n = case.k_chunk + max(case.splits, 1)
    return gamma(n) * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T)


def _g(name, M, N, K, **kw):
    return GemmCase(name, M, N, K, **kw)


_LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]


def _gemm_cases():
    cs = []
    # rtk_gemm_f32: M, N from {1, 31, 127, 128, 129, 257} and K from {1, 2, 7, 8, 9, 15, 16, 17, 33, 157, 1000},
    # every value at least once, every layout at several of them; aligned operands (pads keep ld % 4 == 0)
    shapes = [(1, 1, 1), (31, 127, 2), (127, 31, 7), (128, 128, 8), (129, 257, 9), (257, 129, 15), (128, 1, 16),
              (1, 257, 17), (31, 129, 33), (257, 128, 157), (127, 127, 1000), (129, 31, 16)]
    for i, (M, N, K) in enumerate(shapes):
        ak, bk = _LAYOUTS[i % 4]
        # aligned: every stored row starts on a 16-byte boundary (ld % 4 == 0)
        a_len, b_len = (K if ak else M), (K if bk else N)
        cs.append(_g(f"f32_aligned_{M}x{N}x{K}_{ak}{bk}", M, N, K, ak=ak, bk=bk, a_pad=-a_len % 4, b_pad=-b_len % 4))
    for ak, bk in _LAYOUTS:
        # all four layouts at one ragged shape, aligned, in the wide regime (A wide, then B wide)
        cs.append(_g(f"f32_wide12A_{ak}{bk}", 129, 257, 157, ak=ak, bk=bk, regime="wide12", wide="A",
                     a_pad=-(157 if ak else 129) % 4, b_pad=-(157 if bk else 257) % 4))
        cs.append(_g(f"f32_wide20B_{ak}{bk}", 257, 31, 33, ak=ak, bk=bk, regime="wide20", wide="B",
                     a_pad=-(33 if ak else 257) % 4, b_pad=-(33 if bk else 31) % 4))
        # scalar load path, way 1: the base pointer is one float off (ld % 4 == 0 kept)
        cs.append(_g(f"f32_baseoff_{ak}{bk}", 127, 129, 17, ak=ak, bk=bk, a_off=1, b_off=1,
                     a_pad=-(17 if ak else 127) % 4, b_pad=-(17 if bk else 129) % 4))
        # scalar load path, way 2: lda / ldb not a multiple of 4
        cs.append(_g(f"f32_oddld_{ak}{bk}", 257, 127, 33, ak=ak, bk=bk, regime="wide12", wide="B",
                     a_pad=(-(33 if ak else 257) % 4) + 1, b_pad=(-(33 if bk else 127) % 4) + 3))
        # ldc > N (and a C that starts one float off a 16-byte boundary)
        cs.append(_g(f"f32_ldc_{ak}{bk}", 129, 31, 9, ak=ak, bk=bk, ldc_pad=5, c_off=ak))
    # one operand vector-loaded, the other scalar
    cs.append(_g("f32_mixed_vec_scalar", 128, 129, 1000, ak=1, bk=0, regime="wide12", wide="A", b_pad=2))
    # rtk_score_f32: the same product through its own entry (both K-major, ld = c), ragged
    cs.append(_g("score_ragged", 129, 257, 157, regime="wide12", wide="B", entry="score", ldc_pad=3))
    cs.append(_g("score_small_c", 31, 127, 7, entry="score"))
    # rtk_gemm_f32_splitk
    for s in (1, 2, 7, 16):
        cs.append(_g(f"splitk_s{s}", 129, 31, 1000, ak=1, bk=0, regime="wide12", wide="A", splits=s, b_pad=1))
    # K = 65, 4 splits: k_chunk = 32, the third chunk holds one element, the fourth is empty
    for ak, bk in _LAYOUTS:
        cs.append(_g(f"splitk_partial_empty_{ak}{bk}", 96, 40, 65, ak=ak, bk=bk, splits=4, a_pad=3 if ak else 0))
    cs.append(_g("splitk_mn_mod4", 31, 7, 157, ak=0, bk=0, splits=7, regime="wide12", wide="B"))     # M * N % 4 = 1
    cs.append(_g("splitk_c_off", 127, 33, 157, ak=1, bk=1, splits=2, c_off=1, a_pad=3, b_pad=3))     # scalar reduction
    cs.append(_g("splitk_c_off_mod4", 31, 7, 33, ak=0, bk=1, splits=16, c_off=1))                    # 16 splits, 3 chunks used
    cs.append(_g("splitk_k40943_wide12", 96, 40, 40943, ak=1, bk=0, regime="wide12", wide="A", splits=16, a_pad=1))
    cs.append(_g("splitk_k40943_wide20", 40, 129, 40943, ak=0, bk=0, regime="wide20", wide="B", splits=7))
    cs.append(_g("splitk_k20011_small", 257, 40, 20011, ak=1, bk=0, splits=7, a_pad=1))
    # real-valued layer: K <= 256, each layout, aligned and unaligned
    for ak, bk in _LAYOUTS:
        cs.append(_g(f"real_aligned_{ak}{bk}", 129, 127, 256, ak=ak, bk=bk, regime="real",
                     a_pad=-(256 if ak else 129) % 4, b_pad=-(256 if bk else 127) % 4))
        cs.append(_g(f"real_unaligned_{ak}{bk}", 257, 31, 157, ak=ak, bk=bk, regime="real", a_off=1, b_pad=1 + (-(157 if bk else 31) % 4)))
    cs.append(_g("real_pow2_rows", 128, 129, 200, ak=1, bk=0, regime="real_pow2"))
    cs.append(_g("real_splitk", 96, 40, 256, ak=1, bk=0, regime="real", splits=4))
    return cs


GEMM_CASES = _gemm_cases()
# the sigmoid epilogue of rtk_gemm_f32: small real-valued cases, compared with float64 1 / (1 + exp(-z))
GEMM_SIGMOID_CASES = [_g("sigmoid_11", 129, 31, 17, ak=1, bk=1, regime="real"),
                      _g("sigmoid_00", 31, 257, 33, ak=0, bk=0, regime="real", ldc_pad=2)]


# -------------------------------------------------------------------------------- stage-1 backward ------
@dataclass(frozen=True)
class BwdCase:
    """One call of rtk_query_vectors_bwd_f32: core (a, b, c), R (n_rel, a), S (n_sub, b), dv (B, c).

    ids: how the batch's ids are laid out, (kind, ...) per table -- see bwd_ids().  `wide`: which operand holds the
    wide integers in the wide regimes ("dv" or "core")."""
    name: str
    B: int
    a: int
    b: int
    c: int
    n_rel: int
    n_sub: int
    regime: str = "small"
    wide: str = "dv"
    rel_ids: tuple = ("random",)
    sub_ids: tuple = ("random",)
    branch: str = ""

    @property
    def exact(self):
        return self.regime in EXACT


def bwd_ids(spec, n, B, rng):
    """The id of every query.
      ("random",)            uniform over [0, n)
      ("distinct",)          all different (n >= B), shuffled, ids 0 and n - 1 included
      ("one", id)            one id on every query
      ("lists", (id, counts, first), ...)
                             each listed id has its first query at `first`; counts[w] of its queries lie in window w,
                             the queries [first + 256 w, first + 256 (w + 1)) -- the windows in which
                             scatter_rows_kernel compacts and unrolls the matches of an id (counts[0] includes the
                             first query itself).  Every other query gets an id of its own."""
    kind = spec[0]
    if kind == "random":
        ids = rng.integers(0, n, size=B)
        ids[0], ids[B - 1] = (0, n - 1) if B > 1 else (n - 1, n - 1)
        return ids.astype(np.int64)
    if kind == "distinct":
        assert n >= B
        ids = rng.choice(np.arange(1, n - 1), size=B, replace=False) if n - 2 >= B else rng.permutation(n)[:B]
        if B >= 2:
            ids[B // 3], ids[B - 1] = 0, n - 1
        return ids.astype(np.int64)
    if kind == "one":
        return np.full(B, spec[1], dtype=np.int64)
    if kind == "lists":
        listed = [s[0] for s in spec[1:]]
        ids = np.full(B, -1, dtype=np.int64)
        for j, counts, first in spec[1:]:
            assert ids[first] < 0 and counts[0] >= 1, "two lists start at one query"
            ids[first] = j
        for j, counts, first in spec[1:]:
            for w, count in enumerate(counts):
                lo, hi = first + 256 * w, min(B, first + 256 * (w + 1))
                free = np.flatnonzero(ids[lo:hi] < 0) + lo
                take = count - (w == 0)
                assert len(free) >= take, "the list does not fit its window"
                ids[rng.choice(free, size=take, replace=False)] = j
        rest = np.flatnonzero(ids < 0)
        pool = np.setdiff1d(np.arange(n), listed)
        assert len(pool) >= len(rest), "not enough ids for the unlisted queries"
        ids[rest] = rng.choice(pool, size=len(rest), replace=False)
        return ids
    raise ValueError(kind)


def window_counts(ids):
    """{id: [matches per 256-query window]} as scatter_rows_kernel forms them: the windows of an id start at its
    first query and step by 256; each window's matches are compacted and added in unrolled groups."""
    ids = np.asarray(ids)
    out = {}
    for j in np.unique(ids):
        first = int(np.flatnonzero(ids == j)[0])
        out[int(j)] = [int(np.sum(ids[base:base + 256] == j)) for base in range(first, len(ids), 256)]
    return out


def _bwd_abs_sums(core, R, S, dv, rel, sub):
    return bwd_ref(np.abs(core), np.abs(R), np.abs(S), np.abs(dv), rel, sub)


def bwd_ref(core, R, S, dv, rel, sub, dtype=np.float64, order="natural", chunks=1):
    """(g_core, g_R, g_S) of the header's formulas in `dtype`.
      g_core = sum_d R[r_d] (x) S[h_d] (x) dv[d];  g_R[u] = sum_{d: r_d = u} G x_1 S[h_d] x_2 dv[d];  g_S likewise.
    order="reversed": queries are added last to first and g_core in `chunks` partial sums (like a split-K)."""
    a, b, c = core.shape
    B = dv.shape[0]
    core, R, S, dv = [np.asarray(x, dtype=dtype) for x in (core, R, S, dv)]
    Rq, Sq = R[rel], S[sub]
    W = (dv @ core.reshape(a * b, c).T).reshape(B, a, b)
    rows_R = np.einsum("dab,db->da", W, Sq).astype(dtype)
    rows_S = np.einsum("dab,da->db", W, Rq).astype(dtype)
    X = (Rq[:, :, None] * Sq[:, None, :]).reshape(B, a * b)
    qs = np.arange(B) if order == "natural" else np.arange(B)[::-1]
    g_core = np.zeros((a * b, c), dtype=dtype)
    for part in np.array_split(qs, chunks):
        if len(part):
            g_core = g_core + (X[part].T @ dv[part]).astype(dtype)
    g_R, g_S = np.zeros(R.shape, dtype=dtype), np.zeros(S.shape, dtype=dtype)
    np.add.at(g_R, rel[qs], rows_R[qs])
    np.add.at(g_S, sub[qs], rows_S[qs])
    return g_core.reshape(a, b, c), g_R, g_S


def bwd_rows(core, R, S, dv, rel, sub):
    """The per-query rows the scatter adds (float64): rows_R (B, a), rows_S (B, b)."""
    a, b, c = core.shape
    W = (dv.astype(np.float64) @ core.reshape(a * b, c).astype(np.float64).T).reshape(-1, a, b)
    return np.einsum("dab,db->da", W, S[sub].astype(np.float64)), np.einsum("dab,da->db", W, R[rel].astype(np.float64))


def bwd_operands(case):
    """(core, R, S, dv, rel_idx, sub_idx).  Exact regimes: the densities of the sparse operands are lowered from 1
    in steps of 0.8 until the three abs-sum matrices stay below 2^24 (asserted)."""
    rng = np.random.default_rng(_seed(case.name))
    a, b, c, B = case.a, case.b, case.c, case.B
    rel = bwd_ids(case.rel_ids, case.n_rel, B, rng)
    sub = bwd_ids(case.sub_ids, case.n_sub, B, rng)
    assert rel.min() >= 0 and rel.max() < case.n_rel and sub.min() >= 0 and sub.max() < case.n_sub
    if not case.exact:
        core = real_values(rng, (a, b, c))
        R = real_values(rng, (case.n_rel, a), pow2_rows=case.regime == "real_pow2")
        S = real_values(rng, (case.n_sub, b))
        dv = real_values(rng, (B, c))
        return core, R, S, dv, rel, sub
    bits = 0 if case.regime == "small" else int(case.regime[4:])
    mag = {"core": 2.0, "R": 2.0, "S": 2.0, "dv": 2.0} if not bits else {"core": 1.0, "R": 1.0, "S": 1.0, "dv": 1.0}
    if bits:
        mag[case.wide] = float(2 ** bits)
    dens = {"core": 1.0, "R": 1.0, "S": 1.0, "dv": 1.0}
    L_R = int(np.bincount(rel).max())
    L_S = int(np.bincount(sub).max())
    target = LIMIT / 4          # on the expected sum; the real maximum is asserted below
    for _ in range(200):
        e = {k: dens[k] * mag[k] for k in dens}
        over = []
        if B * e["R"] * e["S"] * e["dv"] > target:
            over += ["R", "S", "dv"]
        if L_S * a * c * e["core"] * e["R"] * e["dv"] > target:
            over += ["core", "R", "dv"]
        if L_R * b * c * e["core"] * e["S"] * e["dv"] > target:
            over += ["core", "S", "dv"]
        if not over:
            break
        for k in set(over):
            if not (bits and k == case.wide):
                dens[k] *= 0.8
    else:
        raise AssertionError(f"{case.name}: no density meets the 2^24 condition -- reshape the case")

    def make(k, shape):
        if bits and k == case.wide:
            return wide_ints(rng, shape, bits)
        return signs(rng, shape, dens[k]) if bits else small_ints(rng, shape, dens[k])
    core, R, S, dv = make("core", (a, b, c)), make("R", (case.n_rel, a)), make("S", (case.n_sub, b)), make("dv", (B, c))
    worst = max(float(x.max()) for x in _bwd_abs_sums(core, R, S, dv, rel, sub))
    assert worst < LIMIT, f"{case.name}: abs-sum {worst} >= 2^24 -- reshape the case"
    return core, R, S, dv, rel, sub


def bwd_bounds(case, core, R, S, dv, rel, sub, splits):
    """Element-wise gamma_n * (sum of absolute terms), float64: n = B + splits + 1 for g_core (the product
    R * S, a chain over the batch, the slab adds), c + a + len(list) + 2 for g_S and c + b + len(list) + 2 for g_R
    (the chain over c, the chain over a or b, the list, two spare)."""
    s_core, s_R, s_S = _bwd_abs_sums(core, R, S, dv, rel, sub)
    len_R = np.bincount(rel, minlength=case.n_rel).astype(np.float64)[:, None]
    len_S = np.bincount(sub, minlength=case.n_sub).astype(np.float64)[:, None]
    return (gamma(case.B + splits + 1) * s_core, gamma(case.c + case.b + len_R + 2) * s_R,
            gamma(case.c + case.a + len_S + 2) * s_S)


def gcore_splits(B, a, b, c):
    """The split-K factor the library picks for g_core (csrc/rtk_query_bwd.hip, gcore_splits)."""
    tiles = -(-(a * b) // 128) * -(-c // 128)
    return int(max(1, min(16, 256 // tiles, B // 64)))


def _b(name, B, a, b, c, n_rel, n_sub, **kw):
    return BwdCase(name, B, a, b, c, n_rel, n_sub, **kw)


def _bwd_cases():
    cs = []
    # ---- row width, slots path (w <= 128): a and b independently ------------------------------------------
    for a, b in ((1, 100), (2, 128), (7, 1), (100, 2), (128, 7)):
        cs.append(_b(f"slots_a{a}_b{b}", 300, a, b, 8, 5, 40, regime="wide12", wide="dv", branch="slots path, row widths"))
    # ---- row width, register path (w > 128): a wide `a` as well as a wide `b` ------------------------------
    for a, b in ((129, 256), (257, 6), (4, 512), (513, 3), (3, 768), (769, 2), (2, 1024), (1024, 2), (256, 129)):
        cs.append(_b(f"regs_a{a}_b{b}", 140, a, b, 8, 6, 30, regime="small", branch="register path, row widths"))
    cs.append(_b("regs_a5_b257_wide_core", 200, 5, 257, 12, 4, 50, regime="wide12", wide="core",
                 branch="register path, wide core"))
    # ---- list lengths.  The kernel compacts the matches of an id per 256-query window (windows start at the id's
    #      first query) and unrolls over that window's count: the edges are counts per window, 8 on the register path
    #      and 8 * slots on the slots path.  Each edge is placed in the first window and again in a later one.
    # register path (b = 200): counts 7, 8, 9, 255, 256 in one window, 257 = 256 + 1, and (1, 8), (3, 7), (2, 9)
    cs.append(_b("regs_lists", 2100, 3, 200, 8, 9, 3000, regime="wide12", wide="dv",
                 sub_ids=("lists", (11, (7,), 0), (12, (8,), 1), (13, (9,), 2), (0, (256,), 300), (2999, (255,), 600),
                          (500, (256, 1), 900), (21, (1, 8), 1500), (22, (3, 7), 1501), (23, (2, 9), 1502)),
                 rel_ids=("random",), branch="register path, counts per window 1 / 7 / 8 / 9 / 255 / 256, list of 257"))
    cs.append(_b("regs_list_all", 700, 2, 130, 4, 3, 10, regime="small", sub_ids=("one", 9), rel_ids=("one", 0),
                 branch="register path, one id on every query (length B: windows of 256, 256, 188)"))
    # slots path, w = 40: slots = 6, edge 48 -> 47, 48, 49 (and 97 = two full passes + 1)
    _w40 = lambda i: ("lists", (i, (47,), 0), (i + 1, (48,), 1), (i + 2, (49,), 2), (i + 3, (97,), 3),  # noqa: E731
                      (i + 4, (5, 48), 300), (i + 5, (1, 47), 301), (i + 6, (2, 49), 302))
    cs.append(_b("slots_lists_w40", 900, 40, 40, 8, 1000, 1000, regime="wide12", wide="core",
                 sub_ids=_w40(1), rel_ids=_w40(990),
                 branch="slots path, counts per window 8 * slots - 1 / 8 * slots / 8 * slots + 1 (slots = 6)"))
    # slots path, w = 128 (b): slots = 2, edge 16 -> 15, 16, 17, 33;  w = 64 (a): slots = 4, edge 32 -> 31, 32, 33, 65
    cs.append(_b("slots_lists_w128_w64", 900, 64, 128, 8, 1200, 1200, regime="small",
                 sub_ids=("lists", (1, (15,), 0), (2, (16,), 1), (3, (17,), 2), (4, (33,), 3), (5, (1, 16), 300),
                          (6, (2, 15), 301), (7, (3, 17), 302)),
                 rel_ids=("lists", (7, (31,), 0), (8, (32,), 1), (9, (33,), 2), (10, (65,), 3), (11, (1, 32), 300),
                          (12, (1, 31), 301), (13, (1, 33), 302)),
                 branch="slots path, counts per window at slots = 2 (edge 16) and slots = 4 (edge 32)"))
    # ---- id placement ----------------------------------------------------------------------------------------
    cs.append(_b("ids_one_relation", 90, 6, 24, 8, 1, 33, regime="wide12", wide="dv", rel_ids=("one", 0),
                 branch="n_rel = 1; ids 0 and n - 1"))
    # 20 significant bits leave room for 16 terms per element: tiny ranks, every id on one query
    cs.append(_b("wide20_dv_tiny", 12, 2, 3, 2, 20, 20, regime="wide20", wide="dv", rel_ids=("distinct",),
                 sub_ids=("distinct",), branch="20-bit dv"))
    cs.append(_b("wide20_core_tiny", 12, 3, 2, 2, 20, 20, regime="wide20", wide="core", rel_ids=("distinct",),
                 sub_ids=("distinct",), branch="20-bit core"))
    cs.append(_b("ids_distinct", 257, 9, 33, 8, 300, 4000, regime="wide12", wide="core", rel_ids=("distinct",),
                 sub_ids=("distinct",), branch="all ids distinct"))
    cs.append(_b("ids_late_first", 600, 5, 72, 8, 900, 900, regime="wide12", wide="dv",
                 sub_ids=("lists", (17, (20,), 560)), rel_ids=("lists", (3, (30,), 530)),
                 branch="first occurrence late in the batch"))
    # ---- batch size, ids in LDS ----------------------------------------------------------------------------
    for B in (1, 255, 256, 257):
        cs.append(_b(f"batch_{B}", B, 6, 40, 8, 4, 50, regime="wide12", wide="dv", branch=f"B = {B}"))
    cs.append(_b("batch_8192", 8192, 4, 16, 8, 11, 3000, regime="small", branch="B = 8192: the last batch with ids in LDS"))
    # ---- batch size above the LDS limit: ids from global memory --------------------------------------------
    cs.append(_b("batch_8193_high_bits", 8193, 4, 16, 8, 3 * 8192, 3 * 8192, regime="small",
                 sub_ids=("lists", (5, (30,), 0), (5 + 8192, (31,), 1), (5 + 16384, (32,), 2)),
                 rel_ids=("lists", (77, (150, 150), 3), (77 + 8192, (145, 145), 7000)),
                 branch="B = 8193 (global ids); ids that differ only above bit 13"))
    cs.append(_b("batch_20000_late_first", 20000, 3, 12, 4, 40000, 40000, regime="small",
                 sub_ids=("lists", (39999, (200, 200, 200, 100), 8200), (0, (33,), 19000)),
                 rel_ids=("lists", (8, (200, 200, 113), 12000), (8 + 8192, (9,), 8192)),
                 branch="B = 20000 (global ids); first occurrences beyond query 8192"))
    cs.append(_b("batch_20000_random", 20000, 3, 10, 4, 7, 500, regime="small",
                 branch="B = 20000, random ids: long lists read from global memory"))
    # ---- gcore_splits ------------------------------------------------------------------------------------------
    cs.append(_b("splits_one", 127, 8, 40, 8, 5, 60, regime="wide12", wide="dv", branch="gcore_splits: B < 128, one split"))
    cs.append(_b("splits_several", 300, 16, 64, 140, 5, 60, regime="wide12", wide="core",
                 branch="gcore_splits: 16 tiles, B = 300 -> 4 splits"))
    cs.append(_b("splits_cap", 1100, 5, 40, 24, 9, 500, regime="wide12", wide="dv", branch="gcore_splits: the cap of 16"))
    # ---- real-valued layer: lists <= 200, c <= 64 ----------------------------------------------------------
    cs.append(_b("real_slots", 400, 10, 40, 40, 5, 300, regime="real", branch="real values, slots path"))
    cs.append(_b("real_regs", 300, 12, 200, 64, 4, 40, regime="real", branch="real values, register path"))
    cs.append(_b("real_pow2", 256, 33, 130, 16, 6, 500, regime="real_pow2", sub_ids=("lists", (3, (200,), 1)),
                 branch="real values, per-row powers of two, one list of 200"))
    return cs


BWD_CASES = _bwd_cases()
# the cases the NULL-output subsets and the workspace refusals run on
BWD_NULL_CASE = _b("null_outputs", 200, 6, 130, 8, 5, 60, regime="wide12", wide="dv", branch="NULL outputs")

