"""The stored-matrix ranking wrappers of ``evaluation.py`` without a GPU: every wrapper that takes ``P`` refuses a CPU
tensor with its own message, and the private helpers they share (the per-row index, the CSR argument triple, the
metrics dictionary) do what the wrappers rely on."""
import re
from types import SimpleNamespace

import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import evaluation as ev

T = torch.tensor([3, 4])
F32 = "P must be a float32 {} GPU tensor with unit column stride"
WRAPPERS = [
    ("filtered_ranks", lambda P: ev.filtered_ranks(P, T), F32.format("(B, N)")),
    ("filtered_ranks bce", lambda P: ev.filtered_ranks(P, T, want_bce=True), F32.format("(B, N)")),
    ("filtered_topk", lambda P: ev.filtered_topk(P, 3),
     "P must be a float32 or bfloat16 (B, n) GPU tensor with unit column stride"),
    ("target_scores_block", lambda P: ev.target_scores_block(P, T, 0), F32.format("(B, n_local)")),
    ("rank_counts_block", lambda P: ev.rank_counts_block(P, T, 0, torch.zeros(2)), F32.format("(B, n_local)")),
    ("tie_counts_block", lambda P: ev.tie_counts_block(P, T, 0, torch.zeros(2)), F32.format("(B, n_local)")),
    ("filtered_tie_counts", lambda P: ev.filtered_tie_counts(P, T), F32.format("(B, N)")),
    ("relation_tie_counts", lambda P: ev.relation_tie_counts(P, T), F32.format("(B, N)")),
]


@pytest.mark.parametrize("name,call,msg", WRAPPERS, ids=[w[0] for w in WRAPPERS])
def test_wrappers_refuse_cpu_scores(name, call, msg):
    for P in (torch.rand(2, 20), torch.rand(0, 20), torch.rand(2, 20).bfloat16()):
        with pytest.raises(RuntimeError, match="^" + re.escape(msg) + "$"):
            call(P)


def test_public_names():
    for name in ("filtered_ranks", "filtered_topk", "filtered_tie_counts", "tie_counts_block"):
        assert getattr(rt, name) is getattr(ev, name)


def test_per_row():
    t = ev._per_row("obj_idx", [[1], [2], [3]], 3, torch.device("cpu"))
    assert t.dtype == torch.int64 and t.shape == (3,) and t.is_contiguous() and t.tolist() == [1, 2, 3]
    pt = ev._per_row("target_scores", torch.zeros(4, dtype=torch.float64)[::2], 2, torch.device("cpu"), torch.float32)
    assert pt.dtype == torch.float32 and pt.is_contiguous()
    assert ev._per_row("obj_idx", [], 0, torch.device("cpu")).numel() == 0
    for name, n in (("obj_idx", 2), ("target_scores", 4), ("keep_idx", 0)):
        with pytest.raises(RuntimeError, match=f"^{name} must have one entry per row of P$"):
            ev._per_row(name, torch.arange(3), n, torch.device("cpu"))


def test_csr_arguments():
    cpu = torch.device("cpu")
    flt = SimpleNamespace(pair_ptr=torch.tensor([0, 2, 3]), pair_obj=torch.tensor([5, 6, 7]),
                          slot_of_item=torch.tensor([1, 0, 1, -1]))
    assert ev._csr(None, 2, cpu) == (None, (None, None, None))
    assert ev._csr(None, 2, cpu, item_ids=torch.arange(2)) == (None, (None, None, None))     # ids without a filter: unused
    slot, ptrs = ev._csr(flt, 3, cpu, item_ids=torch.tensor([3, 0, 1]))
    assert slot.tolist() == [-1, 1, 0] and slot.is_contiguous()
    assert ptrs == (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    slot, ptrs = ev._csr(flt, 2, cpu, slots=[1, -1])                                      # slots win over item_ids
    assert slot.tolist() == [1, -1] and ptrs[0] == slot.data_ptr()
    rows = ev._RowSlots(flt, torch.tensor([0, 1]))                                        # queries that are not items
    assert ev._csr(rows, 2, cpu, item_ids=torch.arange(2))[0].tolist() == [0, 1]
    with pytest.raises(RuntimeError, match="^slots must have one entry per row of P$"):
        ev._csr(flt, 3, cpu, item_ids=torch.arange(2))
    with pytest.raises(ValueError, match="filtering needs the rows' filter slots"):
        ev._csr(flt, 2, cpu)


def test_metrics_dictionary():
    acc5 = [2.0, 1.0, 2.0, 4.0, 99.0]
    assert ev._metrics(acc5, 4) == {"mrr": 0.5, "hits@1": 0.25, "hits@3": 0.5, "hits@10": 1.0}
    assert ev._metrics(acc5[:4], 4) == ev._metrics(acc5, 4)                               # evaluate_relations keeps four
    acc13 = [float(i) for i in range(13)]
    for k, name in enumerate(("optimistic", "realistic", "pessimistic")):
        assert ev._metrics(acc13, 2, name) == {"mrr": 2.0 * k, "hits@1": 2.0 * k + 0.5, "hits@3": 2.0 * k + 1.0,
                                                "hits@10": 2.0 * k + 1.5, "tied": 6.0}
    zero = {"mrr": 0.0, "hits@1": 0.0, "hits@3": 0.0, "hits@10": 0.0}
    assert ev._metrics([0.0] * 5, 0) == zero                                              # an empty dataset divides by 1
    assert ev._metrics([0.0] * 13, 0, "realistic") == dict(zero, tied=0.0)


def test_resolve_device():
    assert ev._resolve_device("cpu") == torch.device("cpu")
    assert ev._resolve_device(torch.device("cuda", 1)) == torch.device("cuda", 1)
