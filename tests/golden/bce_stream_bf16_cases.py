"""Inputs, float64 references, bounds, fp32 emulations, mutants and case lists for the matrix-free BCE loss kernels on
bf16 operands (csrc/rtk_bce_stream_bf16.hip on the skeletons of csrc/rtk_stream_bf16_kernel.h), driven through
rtk_bce_stream_rows_part_bf16 and rtk_bce_stream_grad_o_part_bf16 on bf16 planes packed from a given v
(rtk_pack_query_vectors): no stage 1 and no GEMM enters any bound.  The method is bce_stream_cases.py's (called bs
below); its cases' builder, reference, bounds, verdict, logistics and mutants are imported, and what differs is here.

Operands
  O     exact in bf16: families E and S are bs's as they are (one significant bit, or multiples of 0.5 with at most
        8 significant bits: asserted to survive the rounding to bf16, so the logits stay exact and dz = 0); family G is
        bs's O rounded to bf16, round to nearest even, after its rows were shrunk.
  v     fp32 with full mantissas (family G); the planes hold v^ = bf16(v), round to nearest even.  E and S: v^ = v.

References (float64): z = v^ O^T; rows, x and the positives from z as in bs.reference; dv = X O; gO = X^T (scale v) with
the UNROUNDED v -- the kernel takes the fp32 v of the call, as ops._grads_from_dZ does for bf16 operands.  Data.v is the
unrounded v and Data.z the product of the rounded one, so bs.reference computes exactly that.

Bounds: bs.bounds with one substitution, the chain error of a logit,
    dz = 2^-23 * 16 KS * sum_k |v^_k| |O_jk|       (family G; 0 for E and S),
the bf16 score kernel's bound (tests/test_gpu_score_bf16.py): products of two bf16 values are exact in fp32, the
16 KS partial sums of a row are rounded.  The terms of the two tile products (3 u22 for the splits, the 2^-39
fp16-subnormal floor, the fp32 roundings r_j / r_d, the positives' chains) stay as they are: they hold for x as fp16
hi/lo at 2^14 against one exact fp16 plane of O, and for x as three bf16 terms against O as it is (emul's two routes).
|z| + dz <= 15 outside S and bs.assert_unambiguous hold with that dz (asserted).

The second tile product is cut along the output columns (chunk_columns): the cases' c give one chunk exactly (128), a
chunk and 8 more columns (136, 264), two chunks (256) and four (512); k-step counts 1, 2, 13, 16 (the last two-chain
sum), 17 (the first one-chain sum) and 32.

Mutants: bs.MUTANTS without O_lo_dropped (a bf16 O has no lo half: that mutant is the identity here), and
    go_from_rounded_v          gO formed with v^ instead of v
    x_single_bf16              x rounded to one bf16 in both products
    dv_chunk1_column_dropped   the first column of the second chunk missing from the sweep's dv
    go_chunk1_image_of_chunk0  the second chunk of gO formed with the first chunk's columns of scale v
    loss_per_chunk             the loss partial of the negatives added once per chunk
local_smoothing (t0 = eps / n_local) and positive_in_other_block_counted are bs's block mutants.
tests/test_bce_stream_bf16_cases_host.py shows that the emulations are inside every bound on every case and every
mutant outside on at least one; tests/test_gpu_bce_stream_bf16_kernels.py judges the device with bs.verdict.
Host-only (numpy).
"""
from dataclasses import dataclass
from unittest import mock

import numpy as np

import bce_stream_cases as bs
import ce_kernel_cases as cc

Case, PartCase = bs.Case, bs.PartCase
MODES = bs.MODES
F0, F1 = bs.F0, bs.F1
ROUTES = ("x_f16_hi_lo", "x_three_bf16")
NEW_MUTANTS = ("go_from_rounded_v", "x_single_bf16", "dv_chunk1_column_dropped", "go_chunk1_image_of_chunk0",
               "loss_per_chunk")
MUTANTS = tuple(m for m in bs.MUTANTS if m != "O_lo_dropped") + NEW_MUTANTS
BLOCK_MUTANTS = bs.BLOCK_MUTANTS

KS_CASES = [Case("E", 33, 97, 16 * ks) for ks in (1, 2, 13, 16, 17, 32)]
SHAPE_CASES = [Case("G", 129, 97, 16), Case("G", 33, 97, 24, eps=0.0), Case("G", 70, 97, 128), Case("G", 70, 3003, 136),
               Case("E", 129, 3003, 136), Case("G", 33, 3003, 256), Case("G", 129, 3003, 264), Case("G", 70, 3003, 512),
               Case("E", 70, 3003, 512, eps=0.0)]
SIGMA6_CASE = Case("G", 33, 97, 24, sigma=6.0)
UNIT_SCALE_CASE = Case("G", 33, 97, 16, unit_scale=True)
S_CASES = [Case("S", 33, 97, 16), Case("S", 70, 3003, 264), Case("S", 129, 3003, 512)]
CASES = KS_CASES + SHAPE_CASES + [SIGMA6_CASE, UNIT_SCALE_CASE] + S_CASES


def _parts(c):
    base, below = Case("G", 70, 3003, c), Case("G", 70, 3003, c, below=2000)
    return [PartCase(base, (0, 1501, 3003)),                                     # the cut is inside a tile
            PartCase(base, (0, 1000, 1001, 3003)),                               # a block of one row
            PartCase(below, (0, 2000, 3003)),                                    # a block without positives
            PartCase(base, tuple(3003 * i // 8 for i in range(9)))]              # eight near-equal blocks


PART_CASES = _parts(136) + _parts(512) + [PartCase(S_CASES[1], (0, 1501, 3003))]
MUTANT_PART = PartCase(Case("G", 33, 64, 24, eps=0.5), (0, 32, 64))              # n_ent 64 in two blocks of 32
MUTANT_CASES = [S_CASES[0], S_CASES[1], SIGMA6_CASE, UNIT_SCALE_CASE] + \
    [k for k in SHAPE_CASES if (k.family, k.c) in (("G", 136), ("G", 256), ("G", 264))]


def chunk_columns(c):
    """(chunks, columns of a chunk): the 32-column tiles dealt evenly to the fewest chunks of at most four."""
    nct = -(-((c + 15) // 16) // 2)
    nch = -(-nct // 4)
    return nch, 32 * -(-nct // nch)


# ---------------------------------------------------------------------------------------------- operands --
def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_bits(x):
    """The 16 bits of bf16-exact float32 values."""
    assert np.array_equal(bf16_round(x), x)
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


@dataclass(frozen=True)
class Data(cc.StreamData):
    """v: the fp32 query vectors (unrounded), O: bf16-exact, z = vh O^T (float64), vh = bf16(v)."""
    vh: np.ndarray = None


def operands(case):
    base = bs.operands(case)
    O = bf16_round(base.O) if case.family == "G" else base.O
    vh = bf16_round(base.v)
    if case.family != "G":
        assert np.array_equal(vh, base.v) and np.array_equal(bf16_round(O), O), f"{case.name}: an operand is not exact in bf16"
    return Data(base.csr, base.v, O, vh.astype(np.float64) @ O.astype(np.float64).T, vh)


def chain_bound(case, data):
    if case.family != "G":
        return np.zeros((case.B, case.N))
    return 2.0 ** -23 * 16 * case.ks * (np.abs(data.vh.astype(np.float64)) @ np.abs(data.O.astype(np.float64)).T)


def _own_chain():
    """bs's functions with this module's chain bound."""
    return mock.patch.object(bs, "chain_bound", chain_bound)


def assert_unambiguous(case, data):
    with _own_chain():
        bs.assert_unambiguous(case, data)


def assert_exact(case, data):
    """Families E and S: bs.assert_exact on the rounded operands, which are the operands."""
    bs.assert_exact(case, cc.StreamData(data.csr, data.vh, data.O, data.z))


def bounds(case, data, fast):
    with _own_chain():
        return bs.bounds(case, data, fast)


verdict = bs.verdict
scale_of = bs.scale_of


# ---------------------------------------------------------------------------------------------- reference -
def _link(case, data):
    """float64 (x of the negatives, dt on the unsaturated positives, the negatives' loss rows)."""
    t0, dt = [float(q) for q in bs.consts(case)]
    s1, s0 = bs.saturated(data.z)
    sat = s1 | s0
    x = np.where(sat, 0.0, bs.sc.sigmoid64(data.z) - t0)
    y = np.where(bs.positives_mask(case, data.csr) & ~sat, dt, 0.0)
    lp, lq = bs._logs(data.z)
    return x, y, -(t0 * lp + (1.0 - t0) * lq).sum(axis=1)


def reference(case, data, mutant=None, cuts=None):
    """bs.reference on (v, O, z = v^ O^T), or one of NEW_MUTANTS (whole range only)."""
    if mutant not in NEW_MUTANTS:
        return bs.reference(case, data, mutant, cuts)
    assert cuts is None
    ref = bs.reference(case, data)
    x, y, neg_rows = _link(case, data)
    O64 = data.O.astype(np.float64)
    s = float(scale_of(case))
    sv = s * data.v.astype(np.float64)
    nch, cw = chunk_columns(case.c)
    rows, dv, gO = ref["rows"].copy(), ref["dv"].copy(), ref["gO"].copy()
    if mutant == "go_from_rounded_v":
        gO = (x - y).T @ (s * data.vh.astype(np.float64))
    elif mutant == "x_single_bf16":
        xm = bf16_round(x.astype(np.float32)).astype(np.float64)
        dv, gO = xm @ O64 - y @ O64, xm.T @ sv - y.T @ sv
    elif mutant == "dv_chunk1_column_dropped" and nch > 1:
        dv[:, cw] = -(y @ O64[:, cw])
    elif mutant == "go_chunk1_image_of_chunk0" and nch > 1:
        cols = np.arange(cw, min(2 * cw, case.c))
        gO[:, cols] = x.T @ sv[:, cols - cw] - y.T @ sv[:, cols]
    elif mutant == "loss_per_chunk":
        rows = rows + (nch - 1) * neg_rows
    return dict(rows=rows, dv=dv, gO=gO)


# ---------------------------------------------------------------------------------------------- emulation -
def _three_bf16(y):
    """y (float32) as three bf16 terms, each the rounding of what the ones before leave."""
    a = bf16_round(y)
    b = bf16_round((y - a).astype(np.float32))
    c = bf16_round((y - a - b).astype(np.float32))
    return a, b, c


def emul(case, data, fast, route, perturb=0):
    """bs.emul's rows (the link in numpy fp32 from the fp32 logit), and dv, gO by one of ROUTES:
    x_f16_hi_lo    x at 2^14 as fp16 hi/lo; O as one fp16 plane at the power of two of max |O| (two products), scale v
                   as fp16 hi/lo (three products)
    x_three_bf16   x as three bf16 terms against O as it is (three products) and against scale v as three bf16 terms
                   (the six products of total order <= 2)."""
    rows, _, _ = bs.emul(case, data, fast, perturb)
    t0, dt = bs.consts(case)
    p = bs.logistic32(data.z.astype(np.float32), fast, perturb)
    sat = (p == F1) | (p == F0)
    x = np.where(sat, F0, (p - t0).astype(np.float32)).astype(np.float32)
    Y = np.where(bs.positives_mask(case, data.csr) & ~sat, dt, F0).astype(np.float32)
    sv = (data.v * scale_of(case)).astype(np.float32)
    if route == "x_f16_hi_lo":
        xh, xl = cc._split16(x * np.float32(16384.0))
        sh = cc.pack_shift(np.abs(data.O).max())
        o16 = (data.O * np.float32(2.0 ** sh)).astype(np.float16).astype(np.float32)
        dv = ((xh @ o16 + xl @ o16).astype(np.float32) * np.float32(2.0 ** (-14 - sh))).astype(np.float32)
        shv = cc.pack_shift(np.abs(sv).max())
        th, tl = cc._split16((sv * np.float32(2.0 ** shv)).astype(np.float32))
        gO = ((xh.T @ th + xh.T @ tl + xl.T @ th).astype(np.float32) * np.float32(2.0 ** (-14 - shv))).astype(np.float32)
    else:
        xs, ss = _three_bf16(x), _three_bf16(sv)
        dv = sum((xi @ data.O).astype(np.float32) for xi in xs).astype(np.float32)
        gO = sum((xs[i].T @ ss[j]).astype(np.float32) for i in range(3) for j in range(3 - i)).astype(np.float32)
    return rows, dv - (Y @ data.O).astype(np.float32), gO - (Y.T @ sv).astype(np.float32)


def rows_from_probabilities(case, data, P32):
    """(rows float64, bound) from STORED fp32 probabilities of the same planes and O (the bf16 score kernel's): the loss
    rows of a kernel whose chain and logistic have that kernel's bits.  bs.bounds' rows bound with dz = dp = 0: what is
    left is 1 - p formed in fp32 (u), rtk_clog, the products and the fp32 / float64 sums."""
    U = bs.U
    t0, dt = [float(q) for q in bs.consts(case)]
    p = P32.astype(np.float64)
    s1, s0 = P32 == F1, P32 == F0
    live = ~(s1 | s0)
    with np.errstate(divide="ignore"):
        lp = np.where(s0, -100.0, np.where(s1, 0.0, np.log(np.where(s0, 1.0, p))))
        lq = np.where(s1, -100.0, np.where(s0, 0.0, np.log1p(-np.where(s1, 0.0, p))))
    lp, lq = np.maximum(lp, -100.0), np.maximum(lq, -100.0)
    P = bs.positives_mask(case, data.csr)
    n = data.csr.stored()
    rows = -(t0 * lp + (1.0 - t0) * lq).sum(axis=1) - np.where(P, dt * (lp - lq), 0.0).sum(axis=1)
    alp, alq = np.abs(lp), np.abs(lq)
    Lq = np.where(live, -np.log1p(-U), 0.0)
    mag = t0 * alp + (1.0 - t0) * alq
    neg = t0 * 4 * U * alp * live + U * t0 * alp + (1.0 - t0) * (Lq + 4 * U * alq * live) + 2 * U * (1.0 - t0) * alq \
        + (1 + 16 * 1.01) * U * mag
    pmag = np.where(P, dt * np.abs(lp - lq), 0.0)
    pos = np.where(P, dt * (Lq + 4 * U * (alp + alq) * live), 0.0) + 2 * U * pmag
    bound = neg.sum(axis=1) + pos.sum(axis=1) + (-(-n // 128) + 10) * U * pmag.sum(axis=1) \
        + 2.0 ** -50 * (mag.sum(axis=1) + pmag.sum(axis=1))
    return rows, bound


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
