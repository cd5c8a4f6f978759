"""The three modes of the matrix-free count read the same probabilities: rtk_score_rank_counts_* without and with the
BCE row sums and rtk_score_rank_tie_counts_* on the operands of tests/rank_modes_case.py, the smallest shapes that reach
every branch of step 2 (csrc/rtk_score_rank.hip).  Every figure is an integer count, so every check is exact; the
reference is the numpy tie model (tests/tie_model.py) on the stored score kernel's probabilities."""
import numpy as np
import pytest
import torch

import rank_modes_case
import tie_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _block_counts(rt, cs, lo, hi, pt):
    """The four integer outputs of the three modes on the block [lo, hi), and the BCE row sums."""
    a = (cs.qp, cs.B, cs.O[lo:hi], lo, cs.N, pt, cs.t)
    kw = dict(flt=cs.flt, slots=cs.flt.slot_of_item, sigmoid_mode=cs.mode)
    counts = rt.rank_counts_block_1vN(*a, **kw)
    counts_bce, bce = rt.rank_counts_block_1vN(*a, want_bce=True, **kw)
    greater, equal = rt.rank_tie_counts_block_1vN(*a, **kw)
    assert all(x.dtype == torch.int32 and x.shape == (cs.B,) for x in (counts, counts_bce, greater, equal))
    assert bce.dtype == torch.float64 and torch.isfinite(bce).all()
    return [x.cpu().numpy().astype(np.int64) for x in (counts, counts_bce, greater, equal)]


@pytest.mark.parametrize("kind,mode", [("f32", "fast"), ("f32", "exact"), ("bf16", "exact")])
def test_modes_read_the_same_probabilities(rt, kind, mode):
    cs = rank_modes_case.build(rt, kind, mode)
    B, N, P, tn = cs.B, cs.N, cs.Pn, cs.tn
    # the case is what it says: three finish workgroups, the long list, the empty one, no list, the planted ties
    assert B % 32 != 0 and -(-B // 32) == 3
    assert len(cs.lists[0]) == rank_modes_case.LONG_LIST > 256 and tn[0] in cs.lists[0]
    assert cs.lists[1] == [] and cs.lists[2] is None
    assert P[3, tn[3] - 1] == P[3, tn[3]] == P[3, tn[3] + 1]
    assert P[4, tn[4]] == 0.0 and any(P[4, j] != 0.0 for j in cs.lists[4])
    pt_whole = None
    for blocks in cs.blockings:
        if len(blocks) > 1:
            assert all(any(lo <= j < hi for j in cs.lists[0]) for lo, hi in blocks)
        pt = torch.stack([rt.rank_targets_block(cs.qp, B, cs.O[lo:hi], lo, N, cs.t, sigmoid_mode=mode)
                          for lo, hi in blocks]).max(dim=0).values
        np.testing.assert_array_equal(pt.cpu().numpy(), P[np.arange(B), tn])
        total = np.zeros((4, B), dtype=np.int64)
        for lo, hi in blocks:
            counts, counts_bce, greater, equal = got = _block_counts(rt, cs, lo, hi, pt)
            gt, eq, before = tie_model.tie_counts(P[:, lo:hi], tn, known=cs.lists, col0=lo, pt=pt.cpu().numpy())
            np.testing.assert_array_equal(counts, counts_bce)           # the same with and without bce_rows_out
            np.testing.assert_array_equal(greater + before, counts)     # greater + #{tied ids below t} == counts
            assert ((greater <= counts) & (counts <= greater + equal)).all()
            np.testing.assert_array_equal(greater, gt)
            np.testing.assert_array_equal(equal, eq)
            total += np.stack(got)
        if pt_whole is None:
            pt_whole, whole = pt, total
            assert total[3, 3] >= 2 and total[3, 4] > 0                 # the planted ties are counted as ties
        else:
            assert torch.equal(pt, pt_whole)
            np.testing.assert_array_equal(total, whole)                 # the partition's sums are the whole range's
