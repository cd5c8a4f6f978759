"""A plain numpy model of the tie-aware rank counts (test support, no GPU, no library):

    greater[d] = #{ j != t : p'_j >  p_t }          equal[d] = #{ j != t : p'_j == p_t }

for query d with queried object t, p' = the row with the query's OTHER known-true objects set to 0 (the queried object
keeps its score and is never counted, ids outside the block are skipped), IEEE comparisons (-0 == +0, a NaN never
counts, a NaN p_t gives 0 and 0), and ``before[d] = #{ j < t : p'_j == p_t }``, the part of ``equal`` that the stable
rank ``1 + greater + before`` counts.  Columns are the entities ``col0 + column`` of a block; the counts of the blocks
of a partition add up.

``metrics_sums`` restates ``rtk_tie_metrics_f64`` addition by addition (float64 additions in the kernel's order), so
its sums can be compared with the device's for equality.
"""
import numpy as np

TYPES = ("optimistic", "realistic", "pessimistic")


def filtered(P, obj, known=None, col0=0):
    """p': a copy of the block ``P`` (B, n) with each query's other known-true objects set to 0.  ``known``: None, a
    dense (B, n) array (non-zero = known-true, the reference's targets) or one list of GLOBAL ids per query (None = no
    list)."""
    pf = np.array(P, dtype=np.float32, copy=True)
    B, n = pf.shape
    obj = np.asarray(obj, dtype=np.int64).reshape(-1)
    if known is None:
        return pf
    if isinstance(known, np.ndarray) and known.ndim == 2:
        mask = known != 0
        own = (obj >= col0) & (obj < col0 + n)
        mask[np.nonzero(own)[0], obj[own] - col0] = False
        pf[mask] = 0.0
        return pf
    for d, ids in enumerate(known):
        if ids is None:
            continue
        for g in ids:
            if col0 <= g < col0 + n and g != obj[d]:
                pf[d, g - col0] = 0.0
    return pf


def counts(pf, pt, obj, col0=0):
    """(greater, equal, before), int64 (B,), of the filtered block ``pf`` against the target scores ``pt``."""
    pf = np.asarray(pf, dtype=np.float32)
    obj = np.asarray(obj, dtype=np.int64).reshape(-1, 1)
    pt = np.asarray(pt, dtype=np.float32).reshape(-1, 1)
    ids = col0 + np.arange(pf.shape[1], dtype=np.int64)[None, :]
    with np.errstate(invalid="ignore"):
        gt, eq = pf > pt, pf == pt
    other = ids != obj
    return (gt & other).sum(1), (eq & other).sum(1), (eq & (ids < obj)).sum(1)


def tie_counts(P, obj, known=None, col0=0, pt=None):
    """The model on a block: ``pt`` defaults to the block's own target scores (every ``obj`` inside the block)."""
    P = np.asarray(P, dtype=np.float32)
    obj = np.asarray(obj, dtype=np.int64).reshape(-1)
    if pt is None:
        pt = P[np.arange(P.shape[0]), obj - col0]
    return counts(filtered(P, obj, known, col0), pt, obj, col0)


def ranks(greater, equal, rank_type):
    g, e = np.asarray(greater, dtype=np.float64), np.asarray(equal, dtype=np.float64)
    return 1.0 + g + {"optimistic": 0.0, "realistic": 0.5, "pessimistic": 1.0}[rank_type] * e


def metrics_sums(greater, equal, acc=None):
    """rtk_tie_metrics_f64: acc13 += the batch sums, in the kernel's order of additions -- thread t of 256 adds its
    queries t, t + 256, ... in turn; a wave of 64 sums by the xor butterfly 32, 16, ..., 1; the four waves' sums are
    added from the left, then to the accumulator."""
    g, e = np.asarray(greater, dtype=np.float64).reshape(-1), np.asarray(equal, dtype=np.float64).reshape(-1)
    B = g.size
    v = np.zeros((256, 13), dtype=np.float64)
    for lo in range(0, B, 256):
        m = min(256, B - lo)
        gg, ee = g[lo:lo + m], e[lo:lo + m]
        for k in range(3):
            rk = (1.0 + gg) + (0.5 * k) * ee
            v[:m, 4 * k] += 1.0 / rk
            v[:m, 4 * k + 1] += rk <= 1.0
            v[:m, 4 * k + 2] += rk <= 3.0
            v[:m, 4 * k + 3] += rk <= 10.0
        v[:m, 12] += ee > 0.0
    w = v.reshape(4, 64, 13)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o, :]
    s = w[:, 0, :]
    total = ((s[0] + s[1]) + s[2]) + s[3]
    return (np.zeros(13) if acc is None else np.asarray(acc, dtype=np.float64)) + total


def metrics_of(acc13, rank_type, n):
    """evaluate(rank_type=...)'s dictionary from the 13 sums over n queries."""
    k = 4 * TYPES.index(rank_type)
    return {"mrr": acc13[k] / n, "hits@1": acc13[k + 1] / n, "hits@3": acc13[k + 2] / n, "hits@10": acc13[k + 3] / n,
            "tied": acc13[12] / n}
