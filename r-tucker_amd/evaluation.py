"""Evaluation on the device: the reference's ``evaluate()`` (train.py:94-125) with the
score path and the ranking tail both in HIP.

``evaluate(model, dataset)`` returns the same dictionary the reference returns --
``{"mrr", "hits@1", "hits@3", "hits@10"}`` averaged over the queries, plus the mean BCE
loss -- but never builds the dense (B, N) target matrix on the host and never sorts:
the filter lists of every (subject, relation) pair are uploaded once as a CSR and
``rtk_filtered_rank_f32`` counts the rank of the queried object in one pass over the
score row.  Tie order is that of a stable descending sort (torch's CUDA sort /
``sort(stable=True)``); the reference's default CPU sort is unstable, so on exactly tied
scores its own ranks are implementation-defined.  What can be said about a tied
target on any host is the interval ``[1 + greater, 1 + greater + equal]``:
``filtered_tie_counts`` / ``tie_counts_block`` return the two counts, and
``evaluate(..., rank_type=...)`` the metrics of the optimistic, realistic or pessimistic rank
with the share of tied queries.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .tucker import SFTucker, Tucker


def _resolve_device(device):
    """``device`` as a ``torch.device``, a bare "cuda" as the current CUDA device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class DeviceFilter:
    """The (subject, relation) -> known-true-objects CSR of a ``KG_dataset`` on the device."""

    def __init__(self, dataset, device):
        self.device = torch.device(device)
        # every object of a pair once (the dense targets of Dataset.py:43-50 are idempotent under
        # repeated triples; the kernels that walk the CSR are not)
        ptr, obj = np.asarray(dataset._ptr, dtype=np.int64), np.asarray(dataset._obj, dtype=np.int64)
        seg = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
        key = np.unique(seg * (int(obj.max()) + 1 if len(obj) else 1) + obj)
        m = int(obj.max()) + 1 if len(obj) else 1
        ptr = np.concatenate([[0], np.cumsum(np.bincount(key // m, minlength=len(ptr) - 1))]).astype(np.int64)
        obj = (key % m).astype(np.int64)
        self.max_list = int(np.diff(ptr).max()) if len(ptr) > 1 else 0     # longest list (a host-known bound)
        self.pair_ptr = torch.as_tensor(ptr, device=self.device)
        self.pair_obj = torch.as_tensor(obj, device=self.device)
        f = np.asarray(dataset.features, dtype=np.int64)
        # pair slot of every item, vectorised (a Python loop over the items cost more than the evaluation pass itself):
        # the pairs' (s, r) keys sorted once, the items' keys located by binary search
        if hasattr(dataset, "_pairs"):
            pairs = np.asarray(dataset._pairs, dtype=np.int64).reshape(-1, 2)
        else:                                    # (a dataset that only keeps the (s, r) -> slot dictionary)
            pairs = np.zeros((len(dataset._pair_slot), 2), dtype=np.int64)
            for (s_, r_), i in dataset._pair_slot.items():
                pairs[i] = (s_, r_)
        nr = int(max(pairs[:, 1].max() if len(pairs) else 0, f[:, 1].max() if len(f) else 0)) + 1
        pk = pairs[:, 0] * nr + pairs[:, 1]
        order = np.argsort(pk, kind="stable")
        ik = f[:, 0] * nr + f[:, 1]
        pos = np.searchsorted(pk[order], ik)
        if len(f) and (pos.max(initial=0) >= len(pk) or not np.array_equal(pk[order][np.minimum(pos, len(pk) - 1)], ik)):
            raise KeyError("an item's (subject, relation) pair is not among the dataset's pairs")
        slots = order[pos] if len(f) else np.zeros(0, np.int64)
        self.slot_of_item = torch.as_tensor(slots, device=self.device)
        # the sorted pair keys, for slots_of (queries that are not dataset items)
        self._pair_keys = torch.as_tensor(pk[order], device=self.device)
        self._pair_order = torch.as_tensor(order.astype(np.int64), device=self.device)
        self._key_nr = nr
        self.features = torch.as_tensor(f, device=self.device)
        # contiguous columns: the evaluation loop hands the kernels pointer offsets into them
        self.subj = self.features[:, 0].contiguous()
        self.rel = self.features[:, 1].contiguous()
        self.obj = self.features[:, 2].contiguous() if f.shape[1] > 2 else None
        self._plans = {}

    def slots_of(self, subject_idx, relation_idx) -> torch.Tensor:
        """CSR slot (int64, on the filter's device) of arbitrary (subject, relation) pairs, -1 for a pair the dataset
        does not know: a binary search of the sorted pair keys, no host loop and no host sync."""
        h = torch.as_tensor(subject_idx).to(device=self.device, dtype=torch.int64).reshape(-1)
        r = torch.as_tensor(relation_idx).to(device=self.device, dtype=torch.int64).reshape(-1)
        if h.numel() != r.numel():
            raise RuntimeError(f"subject_idx has {h.numel()} entries, relation_idx {r.numel()}")
        keys = self._pair_keys
        if keys.numel() == 0:
            return torch.full_like(h, -1)
        q = h * self._key_nr + r
        pos = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
        hit = (keys[pos] == q) & (h >= 0) & (r >= 0) & (r < self._key_nr)
        return torch.where(hit, self._pair_order[pos], torch.full_like(q, -1))

    @classmethod
    def of(cls, dataset, device):
        """The filter of ``dataset`` on ``device``, built once per dataset object (``evaluate()`` runs twice per epoch)."""
        device = _resolve_device(device)
        cache = dataset.__dict__.setdefault("_device_filters", {})
        if device not in cache:
            cache[device] = cls(dataset, device)
        return cache[device]


class RelationFilter:
    """The (subject, object) -> known-true-relations CSR of a ``KG_dataset`` on the device: the filter of relation
    prediction, (h, ?, t).  It is built from the triples of the (subject, relation) -> objects lists the dataset holds
    (all splits for a test-mode dataset) and has the fields of a ``DeviceFilter`` -- ``pair_ptr``, ``pair_obj`` (here:
    relation ids, ascending and distinct within a list), ``slot_of_item``, ``features``, ``subj``, ``rel``, ``obj``,
    ``max_list`` -- so ``filtered_ranks``, ``filtered_tie_counts``, ``filtered_topk`` and ``metrics_from_tie_counts`` take
    it as they take a ``DeviceFilter``, with the (B, n_rel) matrix of ``score_relations`` as ``P`` and the relation id as
    the target column."""

    def __init__(self, dataset, device):
        self.device = torch.device(device)
        pairs = np.asarray(dataset._pairs, dtype=np.int64).reshape(-1, 2)
        ptr, obj = np.asarray(dataset._ptr, dtype=np.int64), np.asarray(dataset._obj, dtype=np.int64)
        sr = np.repeat(pairs, np.diff(ptr), axis=0)                        # (s, r) of every held triple
        f = np.asarray(dataset.features, dtype=np.int64)
        ne = int(max(dataset.n_ent, obj.max(initial=-1) + 1, 1))
        nr = int(max(dataset.n_rel, sr[:, 1].max(initial=-1) + 1, 1))
        self._key_ne = ne
        # every (s, o, r) once, sorted by pair key then relation
        key = np.unique((sr[:, 0] * ne + obj) * nr + sr[:, 1])
        pk, rel = key // nr, key % nr
        keys, counts = np.unique(pk, return_counts=True)                   # the pairs, by ascending key: slot = position
        self.pair_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), device=self.device)
        self.pair_obj = torch.as_tensor(rel.astype(np.int64), device=self.device)
        self.max_list = int(counts.max()) if len(counts) else 0
        self._pair_keys = torch.as_tensor(keys.astype(np.int64), device=self.device)
        if f.shape[1] > 2 and len(f):
            ik = f[:, 0] * ne + f[:, 2]
            pos = np.searchsorted(keys, ik)
            if pos.max(initial=0) >= len(keys) or not np.array_equal(keys[np.minimum(pos, len(keys) - 1)], ik):
                raise KeyError("an item's (subject, object) pair is not among the dataset's triples")
            slots = pos.astype(np.int64)
        else:                                                              # (train-mode items are (s, r) pairs: no slot)
            slots = np.full(len(f), -1, dtype=np.int64)
        self.slot_of_item = torch.as_tensor(slots, device=self.device)
        self.features = torch.as_tensor(f, device=self.device)
        self.subj = self.features[:, 0].contiguous()
        self.rel = self.features[:, 1].contiguous()
        self.obj = self.features[:, 2].contiguous() if f.shape[1] > 2 else None
        self._plans = {}

    def slots_of(self, subject_idx, object_idx) -> torch.Tensor:
        """CSR slot (int64, on the filter's device) of arbitrary (subject, object) pairs, -1 for a pair no held triple
        joins: a binary search of the sorted pair keys, no host loop and no host sync."""
        h = torch.as_tensor(subject_idx).to(device=self.device, dtype=torch.int64).reshape(-1)
        t = torch.as_tensor(object_idx).to(device=self.device, dtype=torch.int64).reshape(-1)
        if h.numel() != t.numel():
            raise RuntimeError(f"subject_idx has {h.numel()} entries, object_idx {t.numel()}")
        keys = self._pair_keys
        if keys.numel() == 0:
            return torch.full_like(h, -1)
        q = h * self._key_ne + t
        pos = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
        hit = (keys[pos] == q) & (h >= 0) & (t >= 0) & (t < self._key_ne)
        return torch.where(hit, pos, torch.full_like(q, -1))

    @classmethod
    def of(cls, dataset, device):
        """The relation filter of ``dataset`` on ``device``, built once per dataset object."""
        device = _resolve_device(device)
        cache = dataset.__dict__.setdefault("_relation_filters", {})
        if device not in cache:
            cache[device] = cls(dataset, device)
        return cache[device]


class _RowSlots:
    """A filter's CSR with the rows' slots given directly (queries that are not dataset items): what the ``filtered_*``
    calls read of a filter, with ``item_ids = arange(B)``."""

    def __init__(self, flt, slots):
        self.pair_ptr, self.pair_obj, self.slot_of_item = flt.pair_ptr, flt.pair_obj, slots


def _score_matrix(P, shape, topk=False):
    """The checked score matrix of a ranking call -> ``(B, n, ld, device)``: a float32 GPU matrix with unit column stride
    (``topk``: or bfloat16, and a single column may have any stride).  ``shape``: how the caller's message names it."""
    if (not isinstance(P, torch.Tensor) or not P.is_cuda or P.dim() != 2
            or P.dtype not in ((torch.float32, torch.bfloat16) if topk else (torch.float32,))
            or ((P.shape[1] > 1 or not topk) and P.stride(1) != 1)):
        raise RuntimeError(f"P must be a float32 {'or bfloat16 ' if topk else ''}{shape} GPU tensor with unit column stride")
    return P.shape[0], P.shape[1], P.stride(0), P.device


def _per_row(name, t, B, dev, dtype=torch.int64):
    """``t`` as a flat contiguous ``dtype`` tensor on ``dev`` with one entry per row of P."""
    t = torch.as_tensor(t).to(device=dev, dtype=dtype).contiguous().view(-1)
    if t.numel() != B:
        raise RuntimeError(f"{name} must have one entry per row of P")
    return t


def _csr(flt, B, dev, item_ids=None, slots=None):
    """``(slot, pointers)`` of a call's filter: the rows' CSR slots (from ``slots``, or of the dataset items
    ``item_ids``; the caller keeps the tensor alive) and the ``pair_slot, pair_ptr, pair_obj`` arguments of the C entries
    -- three NULLs without ``flt``."""
    if flt is None:
        return None, (None, None, None)
    if slots is None and item_ids is None:
        raise ValueError("filtering needs the rows' filter slots: item_ids (dataset items) or slots (flt.slots_of)")
    slot = _per_row("slots", slots if slots is not None else flt.slot_of_item[torch.as_tensor(item_ids).to(dev)], B, dev)
    return slot, (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def filtered_ranks(P: torch.Tensor, obj_idx: torch.Tensor, flt: DeviceFilter = None, item_ids: torch.Tensor = None,
                   want_bce: bool = False):
    """Ranks (int32, B) of ``obj_idx`` in the rows of ``P`` after filtering; optionally the per-row BCE sums."""
    lib = _lib.load()
    B, N, ld, dev = _score_matrix(P, "(B, N)")
    obj = _per_row("obj_idx", obj_idx, B, dev)
    ranks = torch.empty(B, dtype=torch.int32, device=dev)
    bce = torch.empty(B, dtype=torch.float64, device=dev) if want_bce else None
    slot, csr = _csr(flt, B, dev, item_ids)
    with torch.cuda.device(dev):
        _lib.check(lib.rtk_filtered_rank_f32(P.data_ptr(), B, N, ld, obj.data_ptr(), *csr, ranks.data_ptr(),
                                             bce.data_ptr() if want_bce else None, _stream(dev)), "rtk_filtered_rank_f32")
    return (ranks, bce) if want_bce else ranks


def filtered_topk(P: torch.Tensor, k: int, flt: DeviceFilter = None, item_ids: torch.Tensor = None,
                  keep_idx: torch.Tensor = None, slots: torch.Tensor = None, col0: int = 0, ids: torch.Tensor = None):
    """The ``k`` best candidates of every row of ``P`` (float32 or bfloat16, (B, n), unit column stride), best first:
    ``(values (B, k) float32, ids (B, k) int64)`` (``rtk_select_topk_*``).  Column j is entity ``col0 + j``, or, with
    ``ids`` (a (B, n) int64 matrix, < 0 = absent), entity ``ids[d, j]`` (merging top-k lists).

    Order of ``torch.sort(descending=True, stable=True)``: equal scores by ascending id; -0.0 == +0.0; NaN above +inf.
    Filtering (``flt``, a ``DeviceFilter``): the row's known-true objects are REMOVED (not set to 0), except
    ``keep_idx[d]`` (-1 = none).  The filter row comes from ``item_ids`` (dataset items) or from ``slots``
    (``flt.slots_of(subject_idx, relation_idx)``; -1 = no filtering).  A row with fewer than k eligible candidates
    is padded with (-inf, -1).  ``P`` is not modified."""
    lib = _lib.load()
    B, n, ld, dev = _score_matrix(P, "(B, n)", topk=True)
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError(f"k = {k}: the selection takes 1 <= k <= 1024")
    if flt is None and (slots is not None or item_ids is not None):
        raise ValueError("slots / item_ids need flt (the DeviceFilter that holds the CSR)")
    slot, csr = _csr(flt, B, dev, item_ids, slots)
    keep = _per_row("keep_idx", keep_idx, B, dev) if keep_idx is not None else None
    if ids is not None:
        if (not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.device != dev
                or tuple(ids.shape) != (B, n) or (n > 1 and ids.stride(1) != 1)):
            raise RuntimeError(f"ids must be an int64 ({B}, {n}) tensor on {dev} with unit column stride")
    values = torch.empty((B, k), dtype=torch.float32, device=dev)
    out_ids = torch.empty((B, k), dtype=torch.int64, device=dev)
    ld = ld if B > 1 else n
    ld_ids = (ids.stride(0) if B > 1 else n) if ids is not None else 0
    fn = lib.rtk_select_topk_bf16 if P.dtype == torch.bfloat16 else lib.rtk_select_topk_f32
    with torch.cuda.device(dev):
        _lib.check(fn(P.data_ptr(), B, n, ld, int(col0), ids.data_ptr() if ids is not None else None, ld_ids, *csr,
                      keep.data_ptr() if keep is not None else None, k, values.data_ptr(), out_ids.data_ptr(), None, 0,
                      _stream(dev)), "rtk_select_topk")
    return values, out_ids


def target_scores_block(P: torch.Tensor, obj_idx: torch.Tensor, col0: int) -> torch.Tensor:
    """Scores of the queried objects that fall into this column block, -inf for the others
    (step 1 of the sharded ranking; all-reduce MAX over the ranks completes it)."""
    lib = _lib.load()
    B, n_loc, ld, dev = _score_matrix(P, "(B, n_local)")
    obj = _per_row("obj_idx", obj_idx, B, dev)
    pt = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.rtk_target_scores_f32(P.data_ptr(), B, n_loc, ld, int(col0), obj.data_ptr(), pt.data_ptr(),
                                             _stream(dev)), "rtk_target_scores_f32")
    return pt


def _counts_block(entry, P, obj_idx, col0, target_scores, flt, item_ids, out0, out1, skip_empty):
    """Step 2 on a stored column block through the C entry ``entry``: the checked operands, the completed target scores
    and the filter's CSR into two (B,) outputs allocated by ``out0`` / ``out1`` (a dtype, or None: NULL)."""
    lib = _lib.load()
    B, n_loc, ld, dev = _score_matrix(P, "(B, n_local)")
    obj = _per_row("obj_idx", obj_idx, B, dev)
    outs = [torch.empty(B, dtype=dt, device=dev) if dt is not None else None for dt in (out0, out1)]
    slot, csr = _csr(flt, B, dev, item_ids)
    pt = _per_row("target_scores", target_scores, B, dev, torch.float32)
    if B > 0 or not skip_empty:                              # (the C entries refuse an empty batch)
        with torch.cuda.device(dev):
            _lib.check(getattr(lib, entry)(P.data_ptr(), B, n_loc, ld, int(col0), pt.data_ptr(), obj.data_ptr(), *csr,
                                           *(o.data_ptr() if o is not None else None for o in outs), _stream(dev)), entry)
    return outs


def rank_counts_block(P: torch.Tensor, obj_idx: torch.Tensor, col0: int, target_scores: torch.Tensor,
                      flt: DeviceFilter = None, item_ids: torch.Tensor = None, want_bce: bool = False):
    """This column block's share of the rank count (int32, B) and, optionally, of the BCE row sums
    (step 2 of the sharded ranking; all-reduce SUM, then rank = 1 + count)."""
    counts, bce = _counts_block("rtk_filtered_rank_partial_f32", P, obj_idx, col0, target_scores, flt, item_ids, torch.int32,
                                torch.float64 if want_bce else None, skip_empty=False)
    return (counts, bce) if want_bce else counts


def tie_counts_block(P: torch.Tensor, obj_idx: torch.Tensor, col0: int, target_scores: torch.Tensor,
                     flt: DeviceFilter = None, item_ids: torch.Tensor = None):
    """This column block's share of the two tie counts (``rtk_filtered_tie_counts_partial_f32``) ->
    ``(greater, equal)`` int32 (B,): the columns j != t of the block with ``p'_j > p_t`` and with ``p'_j == p_t``,
    p' = the row with the query's other known-true objects set to 0.  Arguments as ``rank_counts_block``; the blocks'
    counts add up exactly (all-reduce SUM).  An empty batch gives empty counts."""
    return tuple(_counts_block("rtk_filtered_tie_counts_partial_f32", P, obj_idx, col0, target_scores, flt, item_ids,
                               torch.int32, torch.int32, skip_empty=True))


def filtered_tie_counts(P: torch.Tensor, obj_idx: torch.Tensor, flt: DeviceFilter = None, item_ids: torch.Tensor = None):
    """The tie counts ``(greater, equal)`` (int32, B) of ``obj_idx`` in the rows of ``P`` after filtering: the whole
    matrix as the block ``col0 = 0``.  ``1 + greater <= filtered_ranks <= 1 + greater + equal``."""
    B, _, _, dev = _score_matrix(P, "(B, N)")
    pt = target_scores_block(P, obj_idx, 0) if B > 0 else torch.empty(0, dtype=torch.float32, device=dev)
    return tie_counts_block(P, obj_idx, 0, pt, flt, item_ids)


_TIE_TYPES = ("optimistic", "realistic", "pessimistic")      # the order of rtk_tie_metrics_f64's accumulators


def _check_tie_type(rank_type):
    if rank_type not in _TIE_TYPES:
        raise ValueError(f"rank_type = {rank_type!r}: None (the stable rank), 'optimistic', 'realistic' or 'pessimistic'")


def metrics_from_tie_counts(greater: torch.Tensor, equal: torch.Tensor):
    """Batch SUMS of every tie-aware rank type from the two counts: ``{"optimistic": {"mrr", "hits@1", "hits@3",
    "hits@10"}, "realistic": ..., "pessimistic": ..., "tied": #(equal > 0)}`` (what ``rtk_tie_metrics_f64`` adds up)."""
    from .ops import ranks_from_tie_counts
    out = {}
    for name in _TIE_TYPES:
        r = ranks_from_tie_counts(greater, equal, name)
        out[name] = {"mrr": (1.0 / r).sum(), "hits@1": (r <= 1).sum(), "hits@3": (r <= 3).sum(), "hits@10": (r <= 10).sum()}
    out["tied"] = (torch.as_tensor(equal) > 0).sum()
    return out


def metrics_from_ranks(ranks: torch.Tensor):
    """Batch SUMS like ``src/utils/metrics.py`` (mrr = sum 1/rank, hits@k = #(rank <= k))."""
    r = ranks.to(torch.float64)
    return {"mrr": (1.0 / r).sum(), "hits@1": (ranks <= 1).sum(), "hits@3": (ranks <= 3).sum(),
            "hits@10": (ranks <= 10).sum()}


def _eval_operands(model, device):
    """``(core, R, S, O, sym, device)`` of an evaluation pass: the model's parameters (a symmetric model's entity matrix
    as both S and O) and the device the pass runs on (``device`` or the parameters')."""
    device = _resolve_device(device if device is not None else next(model.parameters()).device)
    sym = hasattr(model, "E")
    S = model.E.weight.data if sym else model.S.weight.data
    return model.core.data, model.R.weight.data, S, S if sym else model.O.weight.data, sym, device


def _add_tie_metrics(lib, greater, equal, nb, acc13, sp):
    """acc13 += the tie-aware metric sums of ``nb`` queries (``rtk_tie_metrics_f64``; arguments are device pointers)."""
    _lib.check(lib.rtk_tie_metrics_f64(greater, equal, nb, acc13, sp), "rtk_tie_metrics_f64")


def _metrics(sums, n, rank_type=None):
    """The metrics dictionary over ``n`` queries from the running sums: of the stable rank (``rtk_rank_metrics_*``'s
    first four) or, with ``rank_type``, that type's four of ``rtk_tie_metrics_f64``'s 13 and the share of tied queries."""
    n = max(n, 1)
    k = 0 if rank_type is None else 4 * _TIE_TYPES.index(rank_type)
    out = {name: sums[k + i] / n for i, name in enumerate(("mrr", "hits@1", "hits@3", "hits@10"))}
    if rank_type is not None:
        out["tied"] = sums[12] / n
    return out


class _EvalPlan:
    """Buffers of one evaluation pass for fixed (batch size, entity count, operand dtype): the score matrix of ONE
    batch (every batch is consumed by the ranking kernel on the same stream before the next one overwrites it),
    ranks, BCE row sums, packed query planes, running sums."""

    def __init__(self, B, N, c, n_rel, dtype, device):
        from .ops import _dtype_code, alloc_scores
        lib = _lib.load()
        self.P = alloc_scores(B, N, device)
        self.ld = self.P.stride(0) if B > 1 else N
        self.ranks = torch.empty(B, dtype=torch.int32, device=device)
        self.bce = torch.empty(B, dtype=torch.float64, device=device)
        self.acc = torch.zeros(5, dtype=torch.float64, device=device)
        self.qp = torch.empty(lib.rtk_packed_query_bytes(_dtype_code(dtype == torch.bfloat16), B, c), dtype=torch.uint8,
                              device=device)
        self.ws_bytes = lib.rtk_from_tables_workspace_bytes(B, n_rel)
        self.ties = None

    def tie_buffers(self):
        """Target scores, the two tie counts and the 13 running sums of ``evaluate(rank_type=...)`` (made on first use)."""
        if self.ties is None:
            B, dev = self.ranks.numel(), self.ranks.device
            self.ties = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                         torch.empty(B, dtype=torch.int32, device=dev), torch.zeros(13, dtype=torch.float64, device=dev))
        return self.ties


@torch.no_grad()
def evaluate(model, dataset, batch_size=512, device=None, flt: DeviceFilter = None, rank_type=None):
    """The reference's ``evaluate`` loop on the device.  ``dataset``: a test-mode ``KG_dataset``.
    Returns (metrics dict averaged over queries, mean BCE loss) like train.py:123-125.

    ``rank_type``: None ranks by the stable rule (the metrics above).  "optimistic", "realistic" or "pessimistic"
    return that tie-aware rank type's ``mrr / hits@1 / hits@3 / hits@10`` instead, plus ``tied``, the share of the
    queries with a competitor at exactly the target's score -- when it is not small, the tie rule and not the model
    decides a stable-rule MRR.  The loss is the same; the tie counts cost one more pass over each batch's scores
    (``rtk_filtered_tie_counts_partial_f32``, ``rtk_tie_metrics_f64``).

    Per batch: stage 1 against the relation tables of the frozen parameters, the score kernel, the filtered-rank
    kernel over the score matrix, the metric sums -- four calls into the C ABI on buffers that are allocated once per
    (dataset, batch size) and reused; the filter CSR is built once per dataset object.  Out-of-range ids are reported
    at the pass's own synchronisation point (reference: IndexError)."""
    from . import ops
    if rank_type is not None:
        _check_tie_type(rank_type)
    core, R, S, O, _, device = _eval_operands(model, device)
    flt = flt or DeviceFilter.of(dataset, device)
    model.eval()          # train.py:96; also drops the relation-table cache: the tables are rebuilt once, below
    n = len(dataset)
    a, b, c = core.shape
    if (b != c or core.dtype not in (torch.float32, torch.bfloat16) or not ops._packed_stage2(c, exact=False)
            or not core.is_cuda
            or any(t.dtype != core.dtype or t.device != core.device or not t.is_contiguous() for t in (R, S, O))):
        return _evaluate_generic(model, dataset, batch_size, device, flt, rank_type)      # (raises what the closure raises)
    lib = _lib.load()
    N, n_rel = O.shape[0], R.shape[0]
    bf16 = core.dtype == torch.bfloat16
    key = (batch_size, N, c, n_rel, core.dtype)
    plan = flt._plans.get(key)
    if plan is None:
        plan = flt._plans[key] = _EvalPlan(min(batch_size, max(n, 1)), N, c, n_rel, core.dtype, device)
    tables = model._cached_tables(core, R) if hasattr(model, "_cached_tables") else None
    if tables is None:
        tables = ops.relation_tables(core, R)
    ft = ops._entry("rtk_query_vectors_from_tables", bf16)
    sp_fn = ops._entry("rtk_score_packed", bf16)
    sflags = ops._score_flags(True, None, torch.float32, bf16)
    with torch.cuda.device(device):
        sp = torch.cuda.current_stream(device).cuda_stream
        ws = ops._workspace(device, sp, plan.ws_bytes)
        plan.acc.zero_()
        P, qp, ranks, bce, acc = (plan.P.data_ptr(), plan.qp.data_ptr(), plan.ranks.data_ptr(), plan.bce.data_ptr(),
                                  plan.acc.data_ptr())
        tp, Sp, Op, wsp, wsn = tables.data_ptr(), S.data_ptr(), O.data_ptr(), ws.data_ptr(), ws.numel()
        hp, rp, op, slp = flt.subj.data_ptr(), flt.rel.data_ptr(), flt.obj.data_ptr(), flt.slot_of_item.data_ptr()
        ptr, objs = flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr()
        if rank_type is not None:
            tie_pt, tie_gt, tie_eq, tie_acc = plan.tie_buffers()
            tie_acc.zero_()
            ptp, gtp, eqp, tap = tie_pt.data_ptr(), tie_gt.data_ptr(), tie_eq.data_ptr(), tie_acc.data_ptr()
        n_batches = 0
        for lo in range(0, n, batch_size):
            nb = min(batch_size, n - lo)
            o8 = 8 * lo
            _lib.check(ft(tp, n_rel, b, c, Sp, S.shape[0], rp + o8, hp + o8, nb, None, qp, wsp, wsn, sp),
                       "rtk_query_vectors_from_tables")
            _lib.check(sp_fn(qp, nb, c, Op, N, P, plan.ld, sflags, sp), "rtk_score_packed")
            _lib.check(lib.rtk_filtered_rank_f32(P, nb, N, plan.ld, op + o8, slp + o8, ptr, objs, ranks, bce, sp),
                       "rtk_filtered_rank_f32")
            # the reference averages the per-batch MEAN losses (train.py:113,125)
            _lib.check(lib.rtk_rank_metrics_scaled_f64(ranks, bce, nb, 1.0 / (nb * N), acc, sp), "rtk_rank_metrics_scaled_f64")
            if rank_type is not None:                        # one more pass over P: the whole matrix as the block col0 = 0
                _lib.check(lib.rtk_target_scores_f32(P, nb, N, plan.ld, 0, op + o8, ptp, sp), "rtk_target_scores_f32")
                _lib.check(lib.rtk_filtered_tie_counts_partial_f32(P, nb, N, plan.ld, 0, ptp, op + o8, slp + o8, ptr, objs,
                                                                   gtp, eqp, sp), "rtk_filtered_tie_counts_partial_f32")
                _add_tie_metrics(lib, gtp, eqp, nb, tap, sp)
            n_batches += 1
    acc = plan.acc.cpu().tolist()
    sums = tie_acc.cpu().tolist() if rank_type is not None else acc
    ops.check_device_errors(device)
    return _metrics(sums, n, rank_type), acc[4] / max(n_batches, 1)


@torch.no_grad()
def _evaluate_generic(model, dataset, batch_size, device, flt, rank_type=None):
    """The same loop through the model's closure (any operand the closure accepts; shapes the fast path does not
    cover end in the closure's own error)."""
    from .ops import check_device_errors, index_check
    if hasattr(model, "E"):
        T = SFTucker(model.core.data, [model.R.weight], num_shared_factors=2, shared_factor=model.E.weight)
    else:
        T = Tucker(model.core.data, [model.R.weight, model.S.weight, model.O.weight])
    n = len(dataset)
    lib = _lib.load()
    acc = torch.zeros(5, dtype=torch.float64, device=device)   # running sums on the device: one sync at the end
    tie_acc = torch.zeros(13, dtype=torch.float64, device=device) if rank_type is not None else None
    n_batches = 0
    # out-of-range ids: checked once, at the loop's own synchronisation point below (reference: IndexError)
    with index_check("deferred"):
        for lo in range(0, n, batch_size):
            hi = min(lo + batch_size, n)
            ids = torch.arange(lo, hi, device=device)
            f = flt.features[lo:hi]
            P = model(f[:, 0], f[:, 1])(T)       # eval mode + no_grad: relation tables built once, reused by every batch
            ranks, bce = filtered_ranks(P, f[:, 2], flt, ids, want_bce=True)
            # the reference averages the per-batch MEAN losses (train.py:113,125): scale this batch's row sums
            bce.mul_(1.0 / (P.shape[0] * P.shape[1]))
            with torch.cuda.device(device):
                _lib.check(lib.rtk_rank_metrics_f64(ranks.data_ptr(), bce.data_ptr(), hi - lo, acc.data_ptr(),
                                                    _stream(device)), "rtk_rank_metrics_f64")
                if rank_type is not None:
                    greater, equal = filtered_tie_counts(P, f[:, 2], flt, ids)
                    _add_tie_metrics(lib, greater.data_ptr(), equal.data_ptr(), hi - lo, tie_acc.data_ptr(), _stream(device))
            n_batches += 1
    acc = acc.cpu().tolist()
    sums = tie_acc.cpu().tolist() if rank_type is not None else acc
    check_device_errors(device)
    return _metrics(sums, n, rank_type), acc[4] / n_batches


@torch.no_grad()
def relation_tie_counts(P: torch.Tensor, relation_idx, flt=None, slots=None):
    """``filtered_tie_counts`` on the (B, n_rel) matrix of ``score_relations`` for queries that are not dataset items:
    ``slots`` = ``flt.slots_of(subject_idx, object_idx)`` of a ``RelationFilter`` (-1 = no list)."""
    if flt is None:
        return filtered_tie_counts(P, relation_idx)
    ids = torch.arange(P.shape[0], device=P.device)
    return filtered_tie_counts(P, relation_idx, _RowSlots(flt, slots), ids)


@torch.no_grad()
def evaluate_relations(model, dataset, batch_size=512, device=None, flt: RelationFilter = None, rank_type=None):
    """``evaluate`` for relation prediction: every triple (h, r, t) of a test-mode ``dataset`` is the query (h, ?, t), r
    is ranked among all relations after the other known relations of (h, t) are filtered out (``RelationFilter``).
    Returns ``(metrics, None)``: the dictionary ``evaluate`` returns -- ``mrr``, ``hits@1``, ``hits@3``, ``hits@10``, plus
    ``tied`` under a ``rank_type`` -- and None in the place of the loss, which this mode does not have.  Per batch:
    ``ops.score_relations`` (no B x a*b intermediate), then the ranking kernels of the stored-matrix path on the
    (B, n_rel) scores.  Out-of-range ids are reported at the pass's own synchronisation point."""
    from . import ops
    if rank_type is not None:
        _check_tie_type(rank_type)
    core, R, S, O, _, device = _eval_operands(model, device)
    flt = flt or RelationFilter.of(dataset, device)
    if flt.obj is None:
        raise RuntimeError("evaluate_relations needs a test-mode dataset: its items are (subject, relation, object) triples")
    model.eval()
    n = len(dataset)
    lib = _lib.load()
    acc = torch.zeros(4, dtype=torch.float64, device=device)
    tie_acc = torch.zeros(13, dtype=torch.float64, device=device) if rank_type is not None else None
    with ops.index_check("deferred"):
        for lo in range(0, n, batch_size):
            hi = min(lo + batch_size, n)
            ids = torch.arange(lo, hi, device=device)
            P = ops.score_relations(core, R, S, O, flt.subj[lo:hi], flt.obj[lo:hi])
            if rank_type is None:
                m = metrics_from_ranks(filtered_ranks(P, flt.rel[lo:hi], flt, ids))
                acc += torch.stack([m["mrr"], m["hits@1"].double(), m["hits@3"].double(), m["hits@10"].double()])
            else:
                greater, equal = filtered_tie_counts(P, flt.rel[lo:hi], flt, ids)
                with torch.cuda.device(device):
                    _add_tie_metrics(lib, greater.data_ptr(), equal.data_ptr(), hi - lo, tie_acc.data_ptr(), _stream(device))
    sums = (acc if rank_type is None else tie_acc).cpu().tolist()
    ops.check_device_errors(device)
    return _metrics(sums, n, rank_type), None
