"""Cases of the bit-exact tests of the stage-1 forward (csrc/rtk_query.hip) and of the packed query planes.

Method (that of exact_cases.py, whose generators are imported): `core`, `R` and `S` are integer-valued, and for
every element the sum of the absolute values of all of its terms stays below 2^24 -- sum_a |R||G| for a table,
sum_b |S| sum_a |R||G| for a query vector.  Every product and every partial sum in any order is then an exactly
representable integer, so tables and vectors have to equal float64 bit for bit on every path:
  VALU tables / contract kernels   fp32 fma chains and fp32 adds of integers;
  bf16 MFMA tables                 operands of at most 8 significant bits, exact products, fp32 sums of integers;
  split-fp16 GEMM tables           operands scaled by one power of two each and split into fp16 hi + lo; exact when
                                   hi + lo holds every element (asserted here on a numpy emulation) and the dropped
                                   lo.lo products are all zero (one operand has no lo half; asserted as well);
  fp32 GEMM with bf16 widening     exact_cases.py's own subject.
Regimes: "small" (all operands in {-2..2}, thinned where a.b is long), "wide12" (core or S holds odd 12-bit
integers, the others sparse signs; fp32 operands only), "wide8" (odd 8-bit integers: what bf16 holds exactly).

Ids carry planted relation counts (rel_ids).  pack_ref / unpack_ref are an independent packer written from the
prose of csrc/rtk_pack.h (the shift from its definition, 2^14 <= max * 2^sh < 2^15).  route() mirrors the host dispatch and names the branches a case reaches;
tests/test_stage1_cases_host.py holds the union over CASES equal to LABELS, and proves the method and a list of
mutants on a numpy emulation of stage 1 (emulate) without a GPU.  Host-only (numpy).

The C ABI requires b == c (the reference's view(-1, b)), so a case has one rank r = b = c; the values the
per-query kernel's b loop would take independently of c (ngroups - 1, 8 ngroups +- 1) are not reachable and are
replaced by the three reachable classes ngroups = 1, 1 < ngroups <= b, ngroups > b (b = 1 and b = 3 are cases).
The grouped contract at c = 1024 is unreachable as well: its LDS, (8 * 1024 + 8 * 1024) * 4 = 65536 bytes, is over
the 64 * 1024 - 1024 plan_contract allows, so B >= 2048 at c = 1024 takes the per-query fallback and is a case of that.
"""
import functools
from dataclasses import dataclass

import numpy as np

from exact_cases import LIMIT, _seed, round_mantissa, signs, small_ints, wide_ints

SENTINEL = -777.25        # output rows nobody may write
GARBAGE = 3.0             # table rows of slots past the batch's distinct relations
PACK_FILL = 0xA5          # packed bytes nobody may write

# ---- constants of the dispatch, with the function or constant of csrc/rtk_query.hip each comes from ----------
GROUPS_LDS_SLOTS = 2048   # GROUPS_LDS_SLOTS: counters in LDS up to this many slots
CH = 8                    # build_groups_impl: CH, ids fetched per thread and trip; `single` = B <= NT * CH
NT_HOSTED, NT_OWN = 256, 1024     # build_groups<256> in tables_kernel / transpose_core_kernel, <1024> in groups_kernel
UT = 4                    # UT: relations per workgroup of tables_kernel
AB = 16                   # tables_kernel: AB, relation-rank slices in flight
VALU_MAX_A = 32           # build_tables: a <= 32, VALU tables
MFMA_MAX_A = 512          # rtk_abi.hip tables_scratch: bf16 MFMA tables up to this a (core_t / r_packed carved)
LB = 8                    # contract_kernel: LB, table rows requested per trip (contract_grouped_kernel: its own LB)
GROUPED_MIN_B = 2048      # plan_contract: QG = 8 and the grouped kernel from this batch size
QG = 8                    # plan_contract: QG
GROUPED_SMEM = 64 * 1024 - 1024   # plan_contract: limit on smem_grouped


@dataclass(frozen=True)
class Stage1Case:
    """B queries, core (a, r, r), R (n_rel, a), S (n_sub, r).  rel_ids: ((relation id, count), ...) planted, the
    rest from the pool of unlisted ids.  wide: the operand that holds the wide integers ("core" or "S").
    parts: the n_parts the _part entry points run with.  entries: "full" = rtk_query_vectors_*, "tables" =
    rtk_relation_tables_* then rtk_query_vectors_from_tables_*."""
    name: str
    B: int
    a: int
    r: int
    n_rel: int
    n_sub: int = 6
    regime: str = "small"
    wide: str = "core"
    rel_ids: tuple = ()
    parts: tuple = ()
    entries: tuple = ("full", "tables")

    @property
    def dtypes(self):
        return ("f32",) if self.regime == "wide12" else ("f32", "bf16")

    @property
    def packed(self):
        return self.r <= 512        # no packed score kernel beyond (rtk_pack_query_vectors refuses c > 512)


# ------------------------------------------------------------------------------------------------ ids ------
def rel_ids(spec, n_rel, B, rng):
    """Relation id of every query: each (id, count) of `spec` holds exactly `count` queries (count 0: the relation
    stays empty).  The other queries take the unlisted ids: every one of them at least once when they fit
    (then uniformly), a random subset of them without repetition otherwise.  Shuffled, so the first occurrence of
    every relation is spread over the batch."""
    listed = [i for i, _ in spec]
    assert len(set(listed)) == len(listed) and all(0 <= i < n_rel for i in listed)
    ids = [np.full(k, i, dtype=np.int64) for i, k in spec]
    rest = B - sum(k for _, k in spec)
    assert rest >= 0, "planted counts exceed the batch"
    pool = np.setdiff1d(np.arange(n_rel), listed)
    if rest:
        assert len(pool), "no relation left for the unplanted queries"
        if len(pool) <= rest:
            ids.append(pool)
            ids.append(rng.choice(pool, size=rest - len(pool)))
        else:
            ids.append(rng.choice(pool, size=rest, replace=False))
    ids = np.concatenate(ids).astype(np.int64)
    rng.shuffle(ids)
    assert len(ids) == B
    return ids


# ------------------------------------------------------------------------------------------- operands ------
def _sf16_halves(x, amax):
    """numpy emulation of the split of rtk_gemm_sf16_splitk: one power-of-two scale from the operand's absolute
    maximum (largest element into [2^14, 2^15)), hi = fp16(x'), lo = fp16(x' - hi).  Returns (x', hi, lo), float64."""
    e = 14 - int(np.floor(np.log2(amax)))
    xs = np.asarray(x, dtype=np.float32) * np.float32(2.0 ** e)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return xs.astype(np.float64), hi.astype(np.float64), lo.astype(np.float64)


@functools.lru_cache(maxsize=None)
def operands(case):
    """(core, R, S, rel_idx, sub_idx): fp32 / int64.  Asserts the 2^24 conditions in float64, what bf16 holds (unless
    wide12) and, for a > 32, what makes the split-fp16 table GEMM exact."""
    rng = np.random.default_rng(_seed("stage1_" + case.name))
    a, r, B = case.a, case.r, case.B
    rel = rel_ids(case.rel_ids, case.n_rel, B, rng)
    zero_row = 1 % case.n_sub
    sub = rng.integers(0, case.n_sub, size=B).astype(np.int64)      # subjects repeat
    sub[0] = 0                                                      # (row 0 is never the zero row)
    if B >= 2:
        sub[B - 1] = case.n_sub - 1
        sub[rng.integers(1, B - 1) if B >= 3 else 1] = zero_row
    bits = 0 if case.regime == "small" else int(case.regime[4:])
    mag = dict(core=1.2, R=1.2, S=1.2) if not bits else dict(core=1.0, R=1.0, S=1.0)
    if bits:
        mag[case.wide] = float(2 ** bits)
    dens = dict(core=1.0, R=1.0, S=1.0)
    while a * r * np.prod([mag[k] * dens[k] for k in dens]) > LIMIT / 8:
        for k in dens:
            if not (bits and k == case.wide):
                dens[k] *= 0.8

    def make(k, shape):
        if bits and k == case.wide:
            return wide_ints(rng, shape, bits)
        return signs(rng, shape, dens[k]) if bits else small_ints(rng, shape, dens[k])
    core, R, S = make("core", (a, r, r)), make("R", (case.n_rel, a)), make("S", (case.n_sub, r))
    # the last term of either sum is visible: the last relation-rank slice and the last subject-rank row are not zero
    R[:, a - 1][R[:, a - 1] == 0] = 1
    S[:, r - 1][S[:, r - 1] == 0] = -1
    z = core[a - 1, r - 1]
    z[z == 0] = 1
    if case.n_sub > 1:
        S[zero_row] = 0
    t_abs = np.abs(R).astype(np.float64) @ np.abs(core).astype(np.float64).reshape(a, r * r)
    assert t_abs.max() < LIMIT, f"{case.name}: table abs-sum {t_abs.max()} >= 2^24"
    v_abs = np.einsum("sb,ubc->usc", np.abs(S).astype(np.float64), t_abs.reshape(-1, r, r)).max()
    assert v_abs < LIMIT, f"{case.name}: vector abs-sum {v_abs} >= 2^24"
    if case.regime != "wide12":
        for x in (core, R, S):
            assert np.array_equal(round_mantissa(x, 8), x), f"{case.name}: not exact in bf16"
    if a > VALU_MAX_A:
        (xr, hr, lr), (xg, hg, lg) = _sf16_halves(R, np.abs(R).max()), _sf16_halves(core, np.abs(core).max())
        assert np.array_equal(hr + lr, xr) and np.array_equal(hg + lg, xg), f"{case.name}: hi + lo != x * scale"
        assert not lr.any() or not lg.any(), f"{case.name}: a dropped lo.lo product is not zero"
    return core, R, S, rel, sub


def reference(case):
    """(tables (n_rel, r, r), v (B, r)) in float64."""
    core, R, S, rel, sub = operands(case)
    T = tables_of(core.astype(np.float64), R.astype(np.float64))
    return T, contract(T, S.astype(np.float64), rel, sub)


def tables_of(core, R, reverse=False):
    """T[u] = sum_a R[u, a] core[a] in the operands' dtype, one relation-rank slice after the other."""
    a = core.shape[0]
    G = core.reshape(a, -1)
    T = np.zeros((R.shape[0], G.shape[1]), dtype=core.dtype)
    for ai in (range(a - 1, -1, -1) if reverse else range(a)):
        T += R[:, ai, None] * G[ai][None, :]
    return T.reshape((R.shape[0],) + core.shape[1:])


def contract(T, S, slot, sub, reverse=False, rows=None):
    """v[d] = sum_b S[sub_d, b] T[slot_d, b, :] in the operands' dtype, one subject-rank row after the other
    (`rows`: the rows that take part, default all).  Evaluated once per distinct (slot, subject) pair."""
    b = T.shape[1]
    rows = np.arange(b) if rows is None else np.asarray(rows)
    rows = rows[::-1] if reverse else rows
    v = np.zeros((len(slot), T.shape[2]), dtype=T.dtype)
    for u in np.unique(slot):
        q = np.flatnonzero(slot == u)
        hs, inv = np.unique(sub[q], return_inverse=True)
        acc = np.zeros((len(hs), T.shape[2]), dtype=T.dtype)
        for bi in rows:
            acc += S[hs, bi, None] * T[u, bi][None, :]
        v[q] = acc[inv]
    return v


# --------------------------------------------------------------------------- packer (from rtk_pack.h) ------
PACK_HDR = 128


def pack_offset(k, row):
    return (((k >> 4) * 2 + ((k >> 3) & 1)) * 32 + row) * 8 + (k & 7)


def pack_shift(mx):
    """Power-of-two shift that brings a row maximum into [2^14, 2^15); 0 for a zero or non-finite row; +-100 at most."""
    if not (mx > 0 and np.isfinite(mx)):
        return 0
    # 2^14 <= mx * 2^sh < 2^15  <=>  sh = 14 - floor(log2 mx)  (float64 log2 of an fp32 number: exact at powers of two, and
    # no fp32 number is within 2^-25 relative of the next one)
    return int(np.clip(14 - int(np.floor(np.log2(np.float64(mx)))), -100, 100))


def bf16_rne(x):
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def pack_layout(B, c, dtype):
    ks = (c + 15) // 16
    planes = 2 if dtype == "f32" else 1
    return ks, planes, PACK_HDR + planes * ks * 1024, (B + 31) // 32


def pack_ref(v, dtype):
    """(bytes, may_write): the packed planes of v (B, c) fp32 as uint8, and the mask of the bytes a producer may
    write (everything but the header entries and plane rows of the rows >= B of the last tile, which stay zero here)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    B, c = v.shape
    ks, planes, tile_bytes, ntiles = pack_layout(B, c, dtype)
    buf = np.zeros(ntiles * tile_bytes, dtype=np.uint8)
    may = np.zeros(ntiles * tile_bytes, dtype=bool)
    k = np.arange(ks * 16)
    vp = np.zeros((B, ks * 16), dtype=np.float32)
    vp[:, :c] = v
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(B):
            tile = buf[(d >> 5) * tile_bytes:(d >> 5) * tile_bytes + tile_bytes]
            tmay = may[(d >> 5) * tile_bytes:(d >> 5) * tile_bytes + tile_bytes]
            row = d & 31
            hdr = tile[:PACK_HDR].view(np.float32)
            pl = tile[PACK_HDR:].view(np.uint16)
            off = pack_offset(k, row)
            if dtype == "f32":
                sh = pack_shift(np.max(np.abs(v[d])))          # (no NaN elements anywhere in these tests)
                hdr[row] = np.float32(2.0 ** -sh)
                x = vp[d] * np.float32(2.0 ** sh)
                hi = x.astype(np.float16)
                lo = (x - hi.astype(np.float32)).astype(np.float16)
                pl[off] = hi.view(np.uint16)
                pl[off + ks * 512] = lo.view(np.uint16)
            else:
                hdr[row] = 1.0
                pl[off] = bf16_rne(vp[d])
            tmay[4 * row:4 * row + 4] = True
            pm = tmay[PACK_HDR:].reshape(-1, 2)
            for p in range(planes):
                pm[off + p * ks * 512] = True
    return buf, may


def unpack_ref(buf, B, c, dtype):
    """The (B, c) values the planes stand for, float64: (hi + lo) * header, or the bf16 plane."""
    ks, planes, tile_bytes, _ = pack_layout(B, c, dtype)
    out = np.zeros((B, c), dtype=np.float64)
    k = np.arange(c)
    for d in range(B):
        tile = buf[(d >> 5) * tile_bytes:(d >> 5) * tile_bytes + tile_bytes]
        row = d & 31
        pl = tile[PACK_HDR:].view(np.uint16)
        off = pack_offset(k, row)
        if dtype == "f32":
            hi = pl[off].view(np.float16).astype(np.float64)
            lo = pl[off + ks * 512].view(np.float16).astype(np.float64)
            with np.errstate(invalid="ignore"):                     # (a clamped row: inf - inf)
                out[d] = (hi + lo) * float(tile[:PACK_HDR].view(np.float32)[row])
        else:
            out[d] = (pl[off].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return out


def _canonical_nan_halves(buf):
    """fp16 NaNs of any sign and payload -> 0x7e00.  The one class of entry the packer test models: the lo half of an
    infinite element is fp16(inf - inf), a NaN whose sign and payload the conversion hardware chooses
    (PACK_SHAPES / pack_rows, the row with an infinite maximum); that it IS a NaN is still asserted."""
    h = buf.copy().view(np.uint16)
    h[(h & 0x7C00 == 0x7C00) & (h & 0x03FF != 0)] = 0x7E00
    return h.view(np.uint8)


def packed_mismatch(got, v, dtype, fill=PACK_FILL, ref=None):
    """None if `got` (uint8, pre-filled with `fill`) holds pack_ref(v) on every byte that may be written and `fill` on
    every other byte; else a message that names the first wrong byte.  ref: pack_ref(v, dtype) if already computed."""
    ref, may = pack_ref(v, dtype) if ref is None else ref
    if len(got) != len(ref):
        return f"{len(got)} packed bytes, expected {len(ref)}"
    B, c = v.shape
    ks, planes, tile_bytes, _ = pack_layout(B, c, dtype)
    want = np.where(may, ref, np.uint8(fill))
    if dtype == "f32" and np.isinf(v).any():
        got, want = _canonical_nan_halves(np.ascontiguousarray(got)), _canonical_nan_halves(want)
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    i = int(bad[0])
    tile, o = divmod(i, tile_bytes)
    if o < PACK_HDR:
        where = f"header of row {tile * 32 + o // 4}"
    else:
        e = (o - PACK_HDR) // 2
        plane, e = divmod(e, ks * 512)
        where = f"plane {plane}, k-step {e // 512}, k-half {(e // 256) & 1}, row {tile * 32 + (e // 8) % 32}, j {e % 8}"
    kind = "may be written" if may[i] else "must stay untouched"
    return f"{len(bad)} packed bytes differ; first at byte {i} ({where}; {kind}): got {got[i]:#04x}, expected {want[i]:#04x}"


# ------------------------------------------------------------------------------- dispatch mirror ------
def plan_contract(b, c, B):
    """(grouped, vec) of plan_contract (csrc/rtk_query.hip) for 16-byte-aligned tables."""
    vec = c % 4 == 0
    W = 4 if vec else 1
    cols = -(-c // W)
    if cols <= 256:
        ng = 256 // cols
        pg = ng - 1 if ng > 1 else 1
        smem = (QG * ((b + 3) & ~3) + QG * pg * cols * W) * 4
    else:
        smem = 1 << 62
    return B >= GROUPED_MIN_B and smem <= GROUPED_SMEM, vec


def dispatch(case, dtype, entry):
    """What the host code decides for one call sequence: a dict the labels and the emulation are derived from."""
    a, b, c, B, n_rel = case.a, case.r, case.r, case.B, case.n_rel
    d = dict(planned=entry == "full" and n_rel > B)
    d["n_slots"] = B if d["planned"] else n_rel
    d["grouped"], d["cvec"] = plan_contract(b, c, B)
    d["groups"] = (d["grouped"] or a > VALU_MAX_A) if entry == "full" else d["grouped"]
    d["qinfo"] = d["groups"] and not d["grouped"]
    if a <= VALU_MAX_A:
        d["tables"], host = ("valu_vec" if (b * c) % 4 == 0 else "valu_scalar"), "tables_kernel"
    elif dtype == "bf16" and a <= MFMA_MAX_A:
        d["tables"], host = "bf16_mfma", "transpose_core_kernel"
    elif dtype == "f32":
        d["tables"], host = ("sf16_gather" if d["planned"] else "sf16_nogather"), "groups_kernel"
    else:
        d["tables"], host = "f32gemm_bf16", "groups_kernel"
    d["host"] = (host if entry == "full" else "groups_kernel") if d["groups"] else None
    d["NT"] = NT_OWN if d["host"] == "groups_kernel" else NT_HOSTED
    W = 4 if d["cvec"] else 1
    d["cols"] = -(-c // W)
    if d["grouped"]:
        d["ngroups"], d["npass"] = 256 // d["cols"], 1
    else:
        d["ngroups"] = 1 if d["cols"] >= 256 else 256 // d["cols"]
        d["npass"] = -(-d["cols"] // 256)
    return d


# the values the issue asks for, per concern: a case that holds one of them reaches the label "<concern>=<value>"
EDGES = {
    "valu_a": (1, 15, 16, 17, 32), "valu_slots": (1, 3, 4, 5),
    "mfma_a": (33, 48, 64, 65, 200, 512), "mfma_slots": (1, 31, 32, 33),
    "sf16_gather_a": (33, 40, 200), "sf16_nogather_a": (33, 40, 200),
    "pq_qinfo_B": (1, 7, 8, 9, 33, 2047), "pq_plain_B": (1, 7, 8, 9, 33, 2047),
    "pq_c": (1, 4, 7, 255, 256, 257, 512, 513, 1020, 1024, 1028), "pq_b": (1, 3),
    "grouped_B": (2048, 2049, 8192, 8193), "grouped_c": (4, 7, 200, 255, 512), "fallback_c": (1024, 1028),
    "grouped_count": (0, 1, 7, 8, 9, 16, 17),
    "groups_in_tables_kernel_slots": (256, 257, 2048, 2049), "groups_in_transpose_core_kernel_slots": (256, 257),
    "groups_in_groups_kernel_full_slots": (1024, 1025), "groups_in_groups_kernel_tables_slots": (1024, 1025, 2049),
    "parts_pq": (2, 3), "parts_grouped": (2, 3),
}
BRANCHES = (
    "planned", "unplanned", "planned_fewer_relations_than_slots", "planned_grouped",
    "tables_valu_vec", "tables_valu_scalar", "tables_bf16_mfma", "tables_sf16_gather", "tables_sf16_nogather",
    "tables_f32gemm_bf16_planned", "tables_f32gemm_bf16_unplanned",
    "transpose_vin", "transpose_scalar_in", "transpose_vout", "transpose_scalar_out",
    "groups_in_tables_kernel", "groups_in_transpose_core_kernel", "groups_in_groups_kernel", "groups_nowhere",
    "counters_lds", "counters_global",
    "single_nt256", "multi_nt256", "single_nt1024", "multi_nt1024",
    "scan_one_chunk_nt256", "scan_chunks_nt256", "scan_one_chunk_nt1024", "scan_chunks_nt1024",
    "contract_grouped", "contract_pq_qinfo", "contract_pq_plain", "contract_pq_fallback",
    "contract_vec", "contract_scalar", "npass_1", "npass_2", "npass_3",
    "pq_ngroups_1", "pq_ngroups_le_b", "pq_ngroups_gt_b", "grouped_ngroups_1", "grouped_ngroups_le_b",
    "grouped_ngroups_gt_b", "grouped_bpad", "grouped_majority_relation",
)
LABELS = frozenset(BRANCHES) | frozenset(f"{k}={v}" for k, vs in EDGES.items() for v in vs)


def route(case, dtype, entry):
    """The branch labels (a subset of LABELS) that `case` reaches with operands of `dtype` through `entry`."""
    d = dispatch(case, dtype, entry)
    a, b, c, B = case.a, case.r, case.r, case.B
    _, _, _, rel, _ = operands(case)
    L = set()

    def edge(concern, value):
        if value in EDGES[concern]:
            L.add(f"{concern}={value}")
    L.add("planned" if d["planned"] else "unplanned")
    n_u = len(np.unique(rel))
    if d["planned"] and n_u < d["n_slots"]:
        L.add("planned_fewer_relations_than_slots")
    if d["planned"] and d["grouped"]:
        L.add("planned_grouped")
    t = d["tables"]
    if t.startswith("valu"):
        edge("valu_a", a)
        edge("valu_slots", d["n_slots"])
    elif t == "bf16_mfma":
        edge("mfma_a", a)
        edge("mfma_slots", d["n_slots"])
        L.add("transpose_vin" if (b * c) % 4 == 0 else "transpose_scalar_in")
        L.add("transpose_vout" if a % 4 == 0 else "transpose_scalar_out")
    elif t.startswith("sf16"):
        edge(t + "_a", a)
    if t == "f32gemm_bf16":
        t += "_planned" if d["planned"] else "_unplanned"
    L.add("tables_" + t)
    if d["groups"]:
        nt = d["NT"]
        L.add("groups_in_" + d["host"])
        who = d["host"] + (("_full" if entry == "full" else "_tables") if d["host"] == "groups_kernel" else "")
        edge(f"groups_in_{who}_slots", d["n_slots"])
        L.add("counters_lds" if d["n_slots"] <= GROUPS_LDS_SLOTS else "counters_global")
        L.add(("single" if B <= nt * CH else "multi") + f"_nt{nt}")
        L.add(("scan_one_chunk" if d["n_slots"] <= nt else "scan_chunks") + f"_nt{nt}")
    else:
        L.add("groups_nowhere")
    L.add("contract_vec" if d["cvec"] else "contract_scalar")
    L.add(f"npass_{d['npass']}")
    ng = d["ngroups"]
    ng_class = "ngroups_1" if ng == 1 else ("ngroups_le_b" if ng <= b else "ngroups_gt_b")
    if d["grouped"]:
        L.add("contract_grouped")
        L.add("grouped_" + ng_class)
        edge("grouped_B", B)
        edge("grouped_c", c)
        if b % 4:
            L.add("grouped_bpad")
        counts = np.bincount(rel, minlength=case.n_rel)
        for k in EDGES["grouped_count"]:
            if np.any(counts == k):
                L.add(f"grouped_count={k}")
        if counts.max() > B // 2:
            L.add("grouped_majority_relation")
        for p in case.parts:
            if entry == "tables":
                edge("parts_grouped", p)
    else:
        L.add("contract_pq_qinfo" if d["qinfo"] else "contract_pq_plain")
        L.add("pq_" + ng_class)
        edge("pq_c", c)
        edge("pq_b", b)
        if B >= GROUPED_MIN_B:
            L.add("contract_pq_fallback")
            edge("fallback_c", c)
        edge("pq_qinfo_B" if d["qinfo"] else "pq_plain_B", B)
        for p in case.parts:
            if entry == "tables":
                edge("parts_pq", p)
    assert L <= LABELS, L - LABELS
    return L


# ------------------------------------------------------------------------------------ emulation ------
def build_groups_emu(slot, sub, n_slots, NT, mutant=None):
    """numpy emulation of build_groups_impl: (order, work, qinfo).  order[pos] = query (-1: never written, the 0xFF
    fill of the workspace), work = [(slot, first position, count)], qinfo[pos] = (subject, query, slot)."""
    B = len(slot)
    sl = slot % 2048 if mutant == "slot_mod_2048" else slot
    cnt = np.bincount(sl, minlength=n_slots)
    fill = np.zeros(n_slots, dtype=np.int64)
    work = {}
    base_q = base_w = prev_q = prev_w = 0
    for s0 in range(0, n_slots, NT):
        nq = cnt[s0:s0 + NT]
        nw = -(-nq // QG)
        bq, bw = (prev_q, prev_w) if mutant == "chunk_base" else (base_q, base_w)
        q0 = bq + np.cumsum(nq) - nq
        w0 = bw + np.cumsum(nw) - nw
        fill[s0:s0 + NT] = q0
        for i in np.flatnonzero(nq):
            for k in range(nw[i]):
                n = min(QG, nq[i] - k * QG)
                if mutant == "drop_last_of_9" and nq[i] % QG == 1 and k == nw[i] - 1:
                    n = 0
                work[int(w0[i]) + k] = (s0 + int(i), int(q0[i]) + k * QG, int(n))
        prev_q, prev_w = base_q, base_w
        base_q, base_w = base_q + int(nq.sum()), base_w + int(nw.sum())
    order = np.full(B, -1, dtype=np.int64)
    qinfo = np.full((B, 3), -1, dtype=np.int64)
    for d in range(B):
        pos = fill[sl[d]]
        fill[sl[d]] += 1
        if pos < B:
            order[pos] = d
            qinfo[pos] = (sub[d], d, sl[d])
    return order, [work[w] for w in range(base_w) if w in work], qinfo


def contract_rows(d, b, mutant=None):
    """The subject-rank rows the contract kernel adds: all of them, or what a mutant leaves."""
    if mutant == "drop_last_b":
        return np.arange(b - 1)
    if mutant == "skip_b_tail":      # the rows of a group's last, partial batch of LB are skipped
        gstep = d["ngroups"] if d["npass"] == 1 else 1
        keep = []
        for g in range(min(gstep, b)):
            rows = np.arange(g, b, gstep)
            keep.append(rows[:len(rows) // LB * LB])
        return np.sort(np.concatenate(keep))
    return np.arange(b)


MUTANTS = ("drop_last_of_9", "chunk_base", "slot_mod_2048", "drop_last_b", "skip_b_tail", "table_past_n_u",
           "wide_11_bits", "wide_8_bits", "part_foreign")


def mutant_applies(mutant, case, dtype, entry):
    d = dispatch(case, dtype, entry)
    _, _, _, rel, _ = operands(case)
    if mutant == "drop_last_of_9":
        return d["grouped"] and bool(np.any(np.bincount(rel) % QG == 1))
    if mutant == "chunk_base":
        return d["groups"] and d["n_slots"] > d["NT"] and bool(np.any(slots_of(case, d) >= d["NT"]))
    if mutant == "slot_mod_2048":
        return d["groups"] and bool(np.any(slots_of(case, d) >= 2048))
    if mutant == "skip_b_tail":
        return len(contract_rows(d, case.r, mutant)) < case.r
    if mutant == "table_past_n_u":
        return d["planned"] and len(np.unique(rel)) < d["n_slots"]
    if mutant in ("wide_11_bits", "wide_8_bits"):
        return case.regime == "wide12"
    if mutant == "part_foreign":
        return bool(case.parts) and entry == "tables"
    return True


def slots_of(case, d):
    """Table slot of every query (planned: the distinct relations in ascending order; the kernel's order is arbitrary)."""
    _, _, _, rel, _ = operands(case)
    return np.searchsorted(np.unique(rel), rel) if d["planned"] else rel


def emulate(case, dtype, entry, mutant=None):
    """Stage 1 as the kernels run it, in float64 on the exact operands: {"v": (B, r), "tables": ..., "parts": {n: [v
    of part 0, ...]}}.  Rows nobody writes hold SENTINEL.  `mutant`: one of MUTANTS."""
    core, R, S, rel, sub = [np.asarray(x, dtype=np.float64) if x.dtype == np.float32 else x for x in operands(case)]
    d = dispatch(case, dtype, entry)
    B, b = case.B, case.r
    if mutant in ("wide_11_bits", "wide_8_bits"):
        keep = 11 if mutant == "wide_11_bits" else 8
        if case.wide == "core":
            core = round_mantissa(core, keep).astype(np.float64)
        else:
            S = round_mantissa(S, keep).astype(np.float64)
    slot = slots_of(case, d)
    if d["planned"]:
        rel_list = np.unique(rel)
        T = np.full((d["n_slots"], b, b), GARBAGE)
        T[:len(rel_list)] = tables_of(core, R[rel_list])
        if mutant == "table_past_n_u":
            slot = np.where(slot == len(rel_list) - 1, len(rel_list), slot)
    else:
        T = tables_of(core, R)
    rows = contract_rows(d, b, mutant)
    out = {"tables": T}

    def run(part=0, parts=1):
        v = np.full((B, b), SENTINEL)
        if d["groups"]:
            order, work, qinfo = build_groups_emu(slot, sub, d["n_slots"], d["NT"], mutant)
        if d["grouped"]:
            qs = [order[q0:q0 + n] for _, q0, n in work]
            ss = [np.full(n, s) for s, _, n in work]
            q, s, h = np.concatenate(qs), np.concatenate(ss), None
            live = q >= 0
            q, s = q[live], s[live]
            h = sub[q]
            mine = s % parts == part
            if mutant == "part_foreign" and parts > 1:
                mine |= s % parts == (part + 1) % parts
        else:
            if d["qinfo"]:
                live = qinfo[:, 1] >= 0
                h, q, s = qinfo[live, 0], qinfo[live, 1], qinfo[live, 2]
            else:
                h, q, s = sub, np.arange(B), slot
            mine = rel[q] % parts == part
            if mutant == "part_foreign" and parts > 1:
                mine |= rel[q] % parts == (part + 1) % parts
        q, s, h = q[mine], s[mine], h[mine]
        if len(q):
            v[q] = contract(T, S, np.minimum(s, len(T) - 1), h, rows=rows)
        return v
    out["v"] = run()
    if entry == "tables":
        out["parts"] = {n: [run(p, n) for p in range(n)] for n in case.parts}
    return out


# ---------------------------------------------------------------------------------------- case list ------
def _c(name, B, a, r, n_rel, **kw):
    return Stage1Case(name, B, a, r, n_rel, **kw)


def _cases():
    cs = []
    # ---- per-query contract, VALU tables (a <= 32): the c list, the a list, slot counts 1 / 3 / 4 / 5, odd b c ----
    # (c = 1024 and 1028 are the two fallback cases below; B = 2047 without qinfo is the from-tables run of qi_a65_r7_B2047)
    cs.append(_c("pq_a1_r1_B1", 1, 1, 1, 1, n_sub=2))                                   # b = c = 1: one term
    cs.append(_c("pq_a15_r4_B7", 7, 15, 4, 3, regime="wide12", wide="S", parts=(2, 3)))
    cs.append(_c("pq_a16_r7_B8", 8, 16, 7, 4, regime="wide8"))
    cs.append(_c("pq_a17_r255_B9", 9, 17, 255, 5, regime="wide12"))
    cs.append(_c("pq_a32_r256_B33", 33, 32, 256, 3, regime="wide8", wide="S"))
    cs.append(_c("pq_a2_r257", 5, 2, 257, 2, regime="wide12", wide="S"))
    cs.append(_c("pq_a3_r512", 6, 3, 512, 2, regime="wide8"))
    cs.append(_c("pq_a2_r513", 5, 2, 513, 2))
    cs.append(_c("pq_a2_r1020", 5, 2, 1020, 2, regime="wide12"))
    # ---- per-query contract with qinfo (a > 32, full path); bf16 MFMA / split-fp16 tables --------------------
    cs.append(_c("qi_a33_B1", 1, 33, 8, 1, n_sub=2, regime="wide8"))
    cs.append(_c("qi_a33_r3_B7_planned", 7, 33, 3, 40, rel_ids=((39, 3),)))             # b = 3 < LB: one partial trip
    cs.append(_c("qi_a40_B8", 8, 40, 8, 5, regime="wide12"))
    cs.append(_c("qi_a40_B9_planned", 9, 40, 8, 100, rel_ids=((99, 2), (0, 2))))
    cs.append(_c("qi_a48_B33_rel32", 33, 48, 8, 32, regime="wide8"))
    cs.append(_c("qi_a64_B40_rel33", 40, 64, 8, 33, regime="wide8", wide="S"))
    cs.append(_c("qi_a65_r7_B2047", 2047, 65, 7, 5, rel_ids=((2, 0), (4, 1500))))
    cs.append(_c("qi_a200_rel3", 12, 200, 8, 3, regime="wide12"))
    cs.append(_c("qi_a200_B31_planned", 31, 200, 8, 50, rel_ids=((49, 4),), regime="wide8", entries=("full",)))
    cs.append(_c("qi_a512_r4", 5, 512, 4, 2, regime="wide8"))
    cs.append(_c("qi_a513_r4", 10, 513, 4, 3, regime="wide8"))
    cs.append(_c("qi_a513_r4_planned", 4, 513, 4, 9, rel_ids=((8, 2),), entries=("full",)))
    # ---- per-query fallback at B >= 2048 (the grouped kernel's LDS does not fit) --------------------------------
    cs.append(_c("fallback_r1028", 2048, 2, 1028, 2, n_sub=4, rel_ids=((1, 9),)))
    cs.append(_c("fallback_r1024", 2048, 2, 1024, 2, n_sub=4, rel_ids=((0, 17),), regime="wide8"))
    # ---- grouped contract: planted counts, group-build hosts, slot-count edges ---------------------------------
    counts = ((2, 0), (3, 1), (4, 7), (5, 8), (6, 9), (7, 16), (8, 17))
    cs.append(_c("g_tables_kernel_256", 2048, 3, 4, 256, n_sub=50, rel_ids=counts + ((255, 1100),), parts=(2, 3)))
    cs.append(_c("g_tables_kernel_257_r7", 2049, 3, 7, 257, n_sub=50, rel_ids=counts + ((256, 9),), regime="wide8"))
    cs.append(_c("g_transpose_256", 2048, 40, 8, 256, n_sub=50, rel_ids=((255, 9), (0, 1)), regime="wide8"))
    cs.append(_c("g_transpose_257", 2049, 40, 8, 257, n_sub=50, rel_ids=((256, 17), (0, 8))))
    cs.append(_c("g_groups_kernel_1024", 8192, 33, 4, 1024, n_sub=3000, rel_ids=((1023, 9), (0, 4200)), regime="wide8"))
    cs.append(_c("g_groups_kernel_1025", 8193, 33, 4, 1025, n_sub=3000, rel_ids=((1024, 9), (1, 0), (1023, 17))))
    cs.append(_c("g_lds_2048", 2048, 3, 4, 2048, n_sub=50, rel_ids=()))
    cs.append(_c("g_global_2049", 2049, 3, 4, 2049, n_sub=50, rel_ids=((2048, 9), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0),
                                                                       (10, 0), (11, 0), (12, 0))))
    cs.append(_c("g_planned_3000", 2049, 3, 4, 3000, n_sub=50, rel_ids=((2999, 9), (0, 17), (1500, 7)), regime="wide12",
                 wide="S"))
    cs.append(_c("g_r200", 2048, 2, 200, 3, n_sub=5, rel_ids=((1, 1), (2, 1400)), regime="wide12"))
    cs.append(_c("g_r255", 2048, 2, 255, 2, n_sub=5, rel_ids=((1, 7),)))
    cs.append(_c("g_r512", 2048, 2, 512, 2, n_sub=5, rel_ids=((0, 8),), regime="wide8", wide="S"))
    return cs


CASES = _cases()
# rtk_pack_query_vectors on planted real-valued rows: (B, c)
PACK_SHAPES = ((1, 1), (31, 8), (32, 9), (33, 16), (31, 17), (33, 200), (32, 512))
# planes of the contract kernels at a real-valued shape: (name, B, a, r, n_rel)
PLANE_CASES = (("planes_pq", 70, 6, 40, 5), ("planes_grouped", 2100, 6, 40, 5))


def pack_rows(B, c, seed):
    """Real-valued fp32 rows with the planted edge rows of the packer test (cycled over the batch): row maxima
    2^-130, 2^-126, 1, 2^100, 2^120, a zero row, a maximum that rounds hi up to 2^15, entries 2^-20 of the maximum, an
    infinite maximum (the non-finite branch of the shift; a NaN maximum cannot arise, the kernels' fmaxf skips NaNs)."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((B, c)) * np.exp(rng.uniform(-6, 0, (B, c)))).astype(np.float32)
    for d in range(B):
        kind = d % 9
        peak = rng.integers(0, c)
        v[d] /= max(np.abs(v[d]).max(), np.float32(1e-30))
        if kind == 0:
            v[d] *= np.float32(2.0 ** -130)
            v[d, peak] = 2.0 ** -130
        elif kind == 1:
            v[d] *= np.float32(2.0 ** -126)
            v[d, peak] = -2.0 ** -126
        elif kind == 2:
            v[d, peak] = 1.0
        elif kind == 3:
            v[d] *= np.float32(2.0 ** 100)
            v[d, peak] = 2.0 ** 100
        elif kind == 4:
            v[d] *= np.float32(2.0 ** 120)
            v[d, peak] = -2.0 ** 120
        elif kind == 5:
            v[d] = 0
        elif kind == 6:
            v[d, peak] = np.nextafter(np.float32(2.0), np.float32(0))      # * 2^14 rounds to 2^15 in fp16
        elif kind == 7:
            v[d] *= np.float32(2.0 ** -20)                                  # fp16-subnormal lo halves
            v[d, peak] = 3.0
        else:
            v[d, peak] = np.inf if d % 2 else -np.inf
    return v
