"""Candidate scoring (``rtk_score_candidates_*``) and its dv (``rtk_score_candidates_bwd_*``, ``dv``): cases,
float64 references with derived bounds, and bit-exact float32 emulations of the order in which the two kernels add.

The forward's order (``include/rtucker_hip.h``; ``cand_fwd_kernel``), flags = 0:

  * w = 4 (fp32) or 8 (bf16) elements make 16 bytes, W = 64 w; a wave holds a row, lane l the elements
    j = i W + l w + q (chunk i < ceil(c / W), q < w), elements j >= c add nothing;
  * a lane adds its products onto +0 by fmaf, i ascending, then q ascending;
  * the 64 lane sums go through s[l] = s[l] + s[l ^ o] for o = 32, 16, 8, 4, 2, 1; every lane ends with the same bits;
  * bf16: v is rounded to bf16 (to nearest, ties to even) first;
  * an id outside [0, n_ent) gives NaN and sets bit 1 of the error word.

The order of dv (``cand_dv_kernel``):

  * quarter = ceil(K / 4); wave w owns the k in [w quarter, min(K, (w + 1) quarter)) -- trailing quarters may be empty;
  * per element j a wave adds fmaf(dz[d, k], O[cand[d, k], j], acc) onto +0 in increasing k and skips the ids outside
    [0, n_ent), whatever their dz;
  * dv[d, j] = ((p0 + p1) + p2) + p3 by plain float32 adds; an empty quarter is +0.

The operands make every product a float32 number, so fmaf is ONE correctly rounded float32 add and both emulations
are chains of ``np.float32`` adds that the kernels have to match bit for bit: dz, v and an fp32 O carry 12 significant
bits (``exact_cases.round_mantissa``); a bf16 O carries 8, and the forward's v, given with 12, is rounded to 8 by the
device.  Exponents are spread over 2^-8 .. 2^8 per factor, so that nearly every add rounds and a change of order
shows in the bits (``tests/test_cand_cases_host.py`` proves that with the mutants below).

Host-only (numpy).
"""
import functools
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from exact_cases import gamma, round_mantissa

SENTINEL = np.float32(-7.0e30)      # padding of dz and of out (ld > K): whoever reads or overwrites it is seen
MAXC = 1024
LANES = 64
F32_RANKS = (1, 3, 4, 5, 252, 256, 260, 512, 516, 768, 772, 1024)
BF16_RANKS = (1, 7, 8, 9, 512, 520, 1020, 1024)
KS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 37)
LABELS = frozenset(
    {f"f32_c{c}" for c in F32_RANKS} | {f"bf16_c{c}" for c in BF16_RANKS} | {f"k{k}" for k in KS}
    | {f"f32_chunks{n}_{e}" for n in (1, 2, 3, 4) for e in ("full", "partial")}
    | {f"bf16_chunks{n}_{e}" for n in (1, 2) for e in ("full", "partial")}
    | {f"{t}_{p}" for t in ("f32", "bf16") for p in ("vector", "scalar_c", "scalar_offset")}
    | {"empty_quarter", "quarter_of_1", "all_quarters_used", "quarter_mult8", "quarter_not_mult8", "quarter_mult4_u4",
       "quarter_not_mult4_u4", "span_split_partial_last", "idle_waves", "own_list", "padded_list", "shared_list",
       "duplicate_ids", "first_row", "last_row", "wide_dz", "wide_out", "v_offset", "dv_offset", "negative_id",
       "id_n_ent", "id_1e12", "nan_dz", "inf_dz", "v_rne_tie", "empty_batch", "empty_k"})


@dataclass(frozen=True)
class CandCase:
    """z (B, K) and dv (B, c) of a (B, K) candidate matrix over O (n_ent, c).  shared: ld_cand = 0, one list for every
    query.  cand_pad / dz_pad / out_pad: ld - K (padding holds the valid id 0 / SENTINEL / SENTINEL).  o_off: ELEMENTS
    by which O is moved off a 16-byte boundary (4 bytes fp32, 2 bytes bf16 each); v_off / dv_off: floats.  bad: the
    invalid ids planted in the lists; dz is NaN there and +inf at the first of them.  kernels: which of the two
    kernels the case runs."""
    name: str
    B: int
    K: int
    c: int
    n_ent: int
    bf16: bool = False
    shared: bool = False
    cand_pad: int = 0
    dz_pad: int = 0
    out_pad: int = 0
    o_off: int = 0
    v_off: int = 0
    dv_off: int = 0
    bad: tuple = ()
    kernels: tuple = ("fwd", "dv")

    @property
    def w(self):
        return 8 if self.bf16 else 4

    @property
    def W(self):
        return LANES * self.w

    @property
    def nch(self):
        return -(-self.c // self.W)

    @property
    def m(self):
        """Elements per lane: the length of a lane's fmaf chain."""
        return self.w * self.nch

    @property
    def vector(self):
        return self.c % self.w == 0 and self.o_off * (2 if self.bf16 else 4) % 16 == 0

    @property
    def in_flight(self):
        """Rows a wave keeps in flight: 8 up to two chunks, 4 above."""
        return 8 if self.nch <= 2 else 4


def quarter_of(K, floor=False):
    return K // 4 if floor else -(-K // 4)


def quarters(K, floor=False):
    """[(k0, k1)] of the four waves.  floor: the mutant -- floor(K / 4), the remainder to the last wave."""
    q = quarter_of(K, floor)
    r = [(min(w * q, K), min((w + 1) * q, K)) for w in range(4)]
    if floor:
        r[3] = (r[3][0], K)
    return r


def span_of(B, K):
    """-> (span, nspan) of the forward: a wave scores `span` candidates of one query.  B K / 16384 rounded up, then
    up to a multiple of 8 (the rows in flight), at most K."""
    span = -(-(B * K) // 16384)
    span = min(-(-span // 8) * 8, K)
    return span, -(-K // span)


def _c(name, B, K, c, n_ent, **kw):
    return CandCase(name, B, K, c, n_ent, **kw)


BAD = (-1, None, 10 ** 12)          # None: n_ent itself
CASES = (
    # ---- fp32: every rank of F32_RANKS once, every K of KS once ------------------------------------------------
    _c("c1_k1", 3, 1, 1, 5),
    _c("c3_k2", 4, 2, 3, 17),
    _c("c4_k3", 5, 3, 4, 17),
    _c("c5_k4", 2, 4, 5, 17),
    _c("c252_k5", 3, 5, 252, 40),
    _c("c256_k7", 5, 7, 256, 40, bad=BAD),                       # batch * nspan = 5: three idle waves in block 1
    _c("c260_k8", 3, 8, 260, 40),
    _c("c512_k9", 3, 9, 512, 40, v_off=1, dv_off=1),
    _c("c516_k31", 2, 31, 516, 60, bad=BAD),
    _c("c768_k32", 2, 32, 768, 60),
    _c("c772_k33", 2, 33, 772, 60, shared=True, bad=BAD),
    _c("c1024_k37", 3, 37, 1024, 97, dz_pad=3, cand_pad=2, out_pad=5),
    # ---- fp32: the quarters of the 8-rows-in-flight kernels; pitches; O off its boundary -------------------------
    _c("c256_k32", 2, 32, 256, 40),
    _c("c252_k33", 2, 33, 252, 40, dz_pad=1, out_pad=1),
    _c("c260_k37", 3, 37, 260, 50, dz_pad=3, cand_pad=2, out_pad=5, bad=BAD),
    _c("c512_k31", 2, 31, 512, 40, shared=True),
    _c("c8_k9_o_off", 4, 9, 8, 33, o_off=1),
    _c("c260_k9_o_off", 3, 9, 260, 33, o_off=1, v_off=3, dv_off=3),
    _c("c768_k7_o_off", 2, 7, 768, 33, o_off=3),
    _c("c4_k33_shared", 6, 33, 4, 200, shared=True, bad=BAD),
    # ---- bf16 ---------------------------------------------------------------------------------------------------
    _c("bf_c1_k1", 3, 1, 1, 5, bf16=True),
    _c("bf_c7_k3", 4, 3, 7, 17, bf16=True),
    _c("bf_c8_k4", 3, 4, 8, 17, bf16=True),
    _c("bf_c9_k5", 3, 5, 9, 17, bf16=True, bad=(-1,)),
    _c("bf_c512_k32", 2, 32, 512, 40, bf16=True),
    _c("bf_c520_k33", 3, 33, 520, 40, bf16=True, dz_pad=2, cand_pad=1, out_pad=3),
    _c("bf_c1020_k7", 5, 7, 1020, 40, bf16=True, bad=BAD),
    _c("bf_c1024_k37", 2, 37, 1024, 60, bf16=True, shared=True, bad=BAD),
    _c("bf_c8_k9_o_off", 4, 9, 8, 33, bf16=True, o_off=1, v_off=1, dv_off=1),
    _c("bf_c520_k31_o_off", 2, 31, 520, 33, bf16=True, o_off=3),
    _c("bf_c512_k2", 3, 2, 512, 40, bf16=True),
    _c("bf_c9_k8", 3, 8, 9, 17, bf16=True),
    # ---- the forward's span split: span 16, 3126 spans per query, the last one holds one entry --------------------
    _c("span_split", 3, 50001, 4, 1000, kernels=("fwd",), out_pad=3),
    _c("bf_span_split", 3, 50001, 4, 1000, bf16=True, kernels=("fwd",)),
    # ---- empty shapes ---------------------------------------------------------------------------------------------
    _c("empty_batch", 0, 5, 8, 40),
    _c("empty_k", 4, 0, 8, 40, out_pad=2),
    _c("bf_empty_k", 4, 0, 8, 40, bf16=True),
)
BY_NAME = {c.name: c for c in CASES}
BOTH_OUTPUTS = {False: "c260_k8", True: "bf_c520_k33"}     # per type: the case that also asks for dv and gO in one call


def cases_of(kernel, bf16=None):
    return [c for c in CASES if kernel in c.kernels and (bf16 is None or c.bf16 == bf16)]


# ------------------------------------------------------------------------------------------- operands -----
def bf16_rne(x):
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_trunc(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_half_up(x):
    """Round to nearest, ties away from zero (add half an ulp of bf16 to the magnitude, truncate)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32)


def _values(rng, shape, bits):
    x = rng.standard_normal(shape) * 2.0 ** rng.uniform(-8, 8, shape)
    x = round_mantissa(x, bits)
    assert np.all(x != 0) and np.all(np.abs(x) > 2.0 ** -40) and np.all(np.abs(x) < 2.0 ** 24)
    return x


def _plant_ties(v):
    """Every third element of v becomes an exact halfway value between two bf16 numbers, the kept bit alternating."""
    u = v.reshape(-1).view(np.uint32)
    pos = np.arange(0, u.size, 3)
    parity = ((pos // 3) % 2).astype(np.uint32)
    u[pos] = (u[pos] & np.uint32(0xFFFE0000)) | (parity << np.uint32(16)) | np.uint32(0x8000)


def bad_ids(case):
    return tuple(case.n_ent if b is None else b for b in case.bad)


@functools.lru_cache(maxsize=None)
def operands(case):
    """-> cand (B or 1, K + cand_pad) int64, dz (B, K + dz_pad) float32, v (B, c) float32, O (n_ent, c) float32 (bf16
    values for a bf16 case), bad_k: the k of the planted invalid ids per row of cand.  Read-only."""
    rng = np.random.default_rng(zlib.crc32(("cand " + case.name).encode()))
    B, K, c, N = case.B, case.K, case.c, case.n_ent
    rows = 1 if case.shared else B
    cand = np.zeros((rows, K + case.cand_pad), dtype=np.int64)              # padding: the valid id 0
    cand[:, :K] = rng.integers(0, N, (rows, K))
    bad_k = np.zeros((rows, len(case.bad)), dtype=np.int64)
    if rows and K:
        cand[0, 0] = 0                                                      # the first and the last row of O
        cand[-1, K - 1] = N - 1
        if K >= 3:
            cand[:, K // 2] = cand[:, 0]                                    # a duplicate inside every row
        free = [k for k in range(K) if k not in (0, K // 2, K - 1)]
        assert len(free) >= len(case.bad), f"{case.name}: no room for the invalid ids"
        for r in range(rows if case.bad else 0):
            bad_k[r] = rng.choice(free, len(case.bad), replace=False)
            cand[r, bad_k[r]] = bad_ids(case)
    dz = np.full((B, K + case.dz_pad), SENTINEL, dtype=np.float32)
    dz[:, :K] = _values(rng, (B, K), 12)
    for i in range(len(case.bad)):                                          # the kernel has to skip these, not add them
        dz[np.arange(B), bad_k[np.arange(B) % max(rows, 1), i]] = np.inf if i == 0 else np.nan
    v = _values(rng, (B, c), 12)
    if case.bf16:
        _plant_ties(v)
    O = _values(rng, (N, c), 8 if case.bf16 else 12)
    if case.bf16:
        assert np.array_equal(bf16_trunc(O), O)
    for a in (cand, dz, v, O, bad_k):
        a.setflags(write=False)
    return SimpleNamespace(cand=cand, dz=dz, v=v, O=O, bad_k=bad_k)


def ids_of(case):
    """-> ids (B, K) int64 as the kernels read them, ok (B, K): inside [0, n_ent)."""
    ids = np.broadcast_to(operands(case).cand[:, :case.K], (case.B, case.K))
    return ids, (ids >= 0) & (ids < case.n_ent)


def forward_v(case, rounding=bf16_rne):
    """The v the forward multiplies with: v itself, or v^ = bf16(v) for a bf16 case."""
    v = operands(case).v
    return rounding(v) if case.bf16 else v


# ---------------------------------------------------------------------------------- float64 references -----
@functools.lru_cache(maxsize=None)
def reference_fwd(case):
    """-> z in float64 (of v^ for bf16; the clamped row for an invalid id, whose entry the kernel makes NaN) and the
    header's bound gamma(m + 6) sum_j |v^_j||o_j|."""
    ids, _ = ids_of(case)
    rows = operands(case).O.astype(np.float64)[np.clip(ids, 0, case.n_ent - 1)]            # (B, K, c)
    v = forward_v(case).astype(np.float64)[:, None, :]
    return (v * rows).sum(-1), gamma(case.m + 6) * (np.abs(v) * np.abs(rows)).sum(-1)


@functools.lru_cache(maxsize=None)
def reference_dv(case):
    """-> dv in float64 and gamma(ceil(K / 4) + 2) sum_k |dz o| per element: the longest path of the tree is a quarter's
    chain, whose first add onto 0 is exact (quarter - 1 roundings), plus the three combine adds."""
    ids, ok = ids_of(case)
    op = operands(case)
    rows = op.O.astype(np.float64)[np.clip(ids, 0, case.n_ent - 1)]                        # (B, K, c)
    g = np.where(ok, op.dz[:, :case.K], 0).astype(np.float64)[:, :, None]
    return (g * rows).sum(1), gamma(quarter_of(case.K) + 2) * (np.abs(g) * np.abs(rows)).sum(1)


# ------------------------------------------------------------------------------------------ emulations -----
def _lane_elements(case, deal, chunks_descending):
    """(m, 64): the element j that lane l adds at step t of its chain (>= c: none)."""
    lane = np.arange(LANES)
    if deal == "contiguous":                            # the mutant: lane l holds j = l m .. l m + m - 1
        return np.stack([lane * case.m + t for t in range(case.m)])
    order = range(case.nch - 1, -1, -1) if chunks_descending else range(case.nch)
    return np.stack([i * case.W + lane * case.w + q for i in order for q in range(case.w)])


def forward_lanes(case, lane_sum="butterfly", deal="strided", chunks_descending=False, rounding=bf16_rne):
    """-> (B K, 64) float32: what each lane of the wave holds after the reduction.  The keyword arguments are the
    mutants."""
    ids, _ = ids_of(case)
    rows = operands(case).O[np.clip(ids, 0, case.n_ent - 1)].reshape(case.B * case.K, case.c)
    prod = np.repeat(forward_v(case, rounding), case.K, axis=0) * rows      # exact: 12 x 12 or 8 x 8 significant bits
    assert prod.dtype == np.float32
    s = np.zeros((case.B * case.K, LANES), dtype=np.float32)
    for j in _lane_elements(case, deal, chunks_descending):
        has = j < case.c
        s[:, has] = s[:, has] + prod[:, j[has]]         # fmaf with an exact product: one rounding
    lane = np.arange(LANES)
    if lane_sum == "sequential":                        # the mutant: lane 0, 1, .. 63 added in turn
        t = s[:, 0]
        for l in range(1, LANES):
            t = t + s[:, l]
        return np.repeat(t[:, None], LANES, axis=1)
    for o in ((32, 16, 8, 4, 2, 1) if lane_sum == "butterfly" else (1, 2, 4, 8, 16, 32)):
        s = s + s[:, lane ^ o]
    assert s.dtype == np.float32
    return s


def emulate_fwd(case, **mutant):
    """out[:, :K] (flags = 0) in the kernel's order; NaN where the id is invalid."""
    _, ok = ids_of(case)
    z = forward_lanes(case, **mutant)[:, 0].reshape(case.B, case.K).copy()
    z[~ok] = np.nan
    return z


def emulate_dv(case, floor=False, descending=False, one_chain=False, pairwise=False, clamp=False):
    """dv (B, c) in the kernel's order, float32.  The keyword arguments are the mutants: floor(K / 4) with the
    remainder to the last wave, decreasing k inside a quarter, one chain over all K, the combine (p0 + p1) + (p2 + p3),
    invalid ids clamped and added instead of skipped."""
    op = operands(case)
    ids, ok = ids_of(case)
    spans = [(0, case.K)] + [(case.K, case.K)] * 3 if one_chain else quarters(case.K, floor)
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k0, k1 in spans:
            acc = np.zeros((case.B, case.c), dtype=np.float32)
            for k in (range(k1 - 1, k0 - 1, -1) if descending else range(k0, k1)):
                prod = op.dz[:, k, None] * op.O[np.clip(ids[:, k], 0, case.n_ent - 1)]     # exact: 12 x 12 or 12 x 8 bits
                use = np.ones(case.B, dtype=bool) if clamp else ok[:, k]
                acc = np.where(use[:, None], acc + prod, acc)
            assert acc.dtype == np.float32
            parts.append(acc)
        p0, p1, p2, p3 = parts
        return (p0 + p1) + (p2 + p3) if pairwise else ((p0 + p1) + p2) + p3


@functools.lru_cache(maxsize=None)
def expected_fwd(case):
    z = emulate_fwd(case)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def expected_dv(case):
    g = emulate_dv(case)
    g.setflags(write=False)
    return g


def expected_error_word(case):
    return 0 if ids_of(case)[1].all() else 2


FWD_MUTANTS = {
    "lane sums added sequentially": lambda case: emulate_fwd(case, lane_sum="sequential"),
    "butterfly o = 1 .. 32": lambda case: emulate_fwd(case, lane_sum="reversed"),
    "elements dealt lane-contiguously": lambda case: emulate_fwd(case, deal="contiguous"),
    "chunks in descending order": lambda case: emulate_fwd(case, chunks_descending=True),
}
FWD_MUTANTS_BF16 = {
    "v truncated to bf16": lambda case: emulate_fwd(case, rounding=bf16_trunc),
    "v rounded half away from zero": lambda case: emulate_fwd(case, rounding=bf16_half_up),
}
DV_MUTANTS = {
    "quarter = floor(K / 4)": lambda case: emulate_dv(case, floor=True),
    "decreasing k inside a quarter": lambda case: emulate_dv(case, descending=True),
    "one chain over all K": lambda case: emulate_dv(case, one_chain=True),
    "pairwise combine": lambda case: emulate_dv(case, pairwise=True),
    "invalid ids clamped and added": lambda case: emulate_dv(case, clamp=True),
}


# ---------------------------------------------------------------------------------------------- coverage -----
def features(case):
    """What of LABELS the case reaches, from its shape and its operands."""
    t = "bf16" if case.bf16 else "f32"
    if case.B == 0:
        return {"empty_batch"}
    if case.K == 0:
        return {"empty_k"}
    f = set()
    op = operands(case)
    ids, ok = ids_of(case)
    if case.c in (BF16_RANKS if case.bf16 else F32_RANKS):
        f.add(f"{t}_c{case.c}")
    f.add(f"{t}_chunks{case.nch}_{'partial' if case.c % case.W else 'full'}")
    f.add(f"{t}_vector" if case.vector else f"{t}_scalar_c" if case.c % case.w else f"{t}_scalar_offset")
    if case.shared:
        f.add("shared_list")
    else:
        f.add("padded_list" if case.cand_pad else "own_list")
    if any(len(set(r.tolist())) < case.K for r in ids):
        f.add("duplicate_ids")
    if (ids == 0).any():
        f.add("first_row")
    if (ids == case.n_ent - 1).any():
        f.add("last_row")
    if (ids < 0).any():
        f.add("negative_id")
    if (ids == case.n_ent).any():
        f.add("id_n_ent")
    if (ids == 10 ** 12).any():
        f.add("id_1e12")
    if "fwd" in case.kernels:
        span, nspan = span_of(case.B, case.K)
        if nspan > 1 and case.K % span:
            f.add("span_split_partial_last")
        if case.B * nspan % 4:
            f.add("idle_waves")
        if case.out_pad:
            f.add("wide_out")
        if case.v_off % 4:
            f.add("v_offset")
        if case.bf16:
            u = op.v.view(np.uint32)
            tie = (u & np.uint32(0xFFFF)) == 0x8000
            if (tie & ((u >> np.uint32(16)) & np.uint32(1) == 0)).any() and (tie & ((u >> np.uint32(16)) & np.uint32(1) == 1)).any():
                f.add("v_rne_tie")
    if "dv" in case.kernels:
        if case.K in KS:
            f.add(f"k{case.K}")
        q = quarter_of(case.K)
        lens = [k1 - k0 for k0, k1 in quarters(case.K)]
        f.add("empty_quarter" if 0 in lens else "all_quarters_used")
        if q == 1:
            f.add("quarter_of_1")
        for n in set(lens) - {0}:
            if case.in_flight == 8:
                f.add("quarter_not_mult8" if n % 8 else "quarter_mult8")
            else:
                f.add("quarter_not_mult4_u4" if n % 4 else "quarter_mult4_u4")
        if case.dz_pad:
            f.add("wide_dz")
        if case.dv_off % 4:
            f.add("dv_offset")
        g = op.dz[:, :case.K]
        if np.isnan(g[~ok]).any():
            f.add("nan_dz")
        if np.isinf(g[~ok]).any():
            f.add("inf_dz")
    return f
