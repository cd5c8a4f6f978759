"""Relation-table cache shared by both model flavours.

``M_r = G x_0 R[r]`` (the einsum of ``R_TuckER.py:45``) is a function of the parameters only.  The
reference's ``evaluate()`` (train.py:94-125) runs ``model.eval()`` under ``torch.no_grad()`` and scores
every batch of the split with the SAME ``extract_tensor(model)``; the closure of a model in that state
builds the tables of all relations once and every following batch only does the subject-mode
contraction.  The cache is dropped whenever the parameters can have changed:

* ``model.train()`` / ``model.eval()`` (the reference switches mode around every training epoch),
  ``init``, ``load_state_dict``, ``.to()`` and friends (``_apply``);
* an in-place update of ``core`` / ``R.weight`` that autograd's version counter sees.

NOT seen: writes through ``.data`` while the model stays in eval mode (``W.data.add_(...)`` does not
bump ``W._version``; the reference's optimizers write that way, but only between ``model.train()`` and
the next ``model.eval()``).  Call ``model.invalidate_tables()`` after such a write, or set
``model.cache_tables = False``.
"""
from __future__ import annotations

import torch

from ..ops import rank_1vN, score_1vN, score_candidates, score_triples, topk_1vN


class TablesCacheMixin:
    cache_tables = True

    def _tables_reset(self):
        self.__dict__["_tables"] = None
        self.__dict__["_tables_key"] = None

    def invalidate_tables(self):
        self._tables_reset()

    def train(self, mode: bool = True):
        self._tables_reset()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self._tables_reset()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._tables_reset()
        return super().load_state_dict(*args, **kwargs)

    def _cached_tables(self, core, R):
        """Tables for ``(core, R)`` if they are this model's own parameters in a frozen state, else None."""
        if (not self.cache_tables or self.training or torch.is_grad_enabled() or not core.is_cuda
                or core.data_ptr() != self.core.data_ptr() or R.data_ptr() != self.R.weight.data_ptr()
                or tuple(core.shape) != tuple(self.core.shape) or core.dtype != self.core.dtype
                or torch.cuda.is_current_stream_capturing()):
            return None
        key = (self.core._version, self.R.weight._version, self.core.data_ptr(), self.R.weight.data_ptr(),
               self.core.dtype, self.core.device)
        if self.__dict__.get("_tables") is None or self.__dict__.get("_tables_key") != key:
            from ..ops import relation_tables
            self.__dict__["_tables"] = relation_tables(self.core.detach(), self.R.weight.detach())
            self.__dict__["_tables_key"] = key
        return self.__dict__["_tables"]


class ObjectQueriesMixin:
    """Object prediction, (h, r, ?), for both model flavours, written once on two hooks of the flavour:
    ``_operands_of(T)`` -> ``(core, R, S, O)`` of a Tucker container (sizes, dtype and device come from T, never from
    ``self.rank``: during training T is the doubled-rank tangent-space construct) and
    ``_relation_operands()`` -> the same four of the model's own parameters.  The symmetric model gives its one entity
    matrix as both S and O; autograd sums the two gradients.  In eval mode the relation tables are cached."""

    def forward(self, subject_idx, relation_idx):
        def score_fn(T):
            core, R, S, O = self._operands_of(T)
            return score_1vN(core, R, S, O, subject_idx, relation_idx, tables=self._cached_tables(core, R))

        return score_fn

    def score_candidates(self, subject_idx, relation_idx, candidates):
        """``score_fn(T)`` giving the (B, K) scores of each query against its own candidate entities
        (``ops.score_candidates``; ``candidates`` int64 (B, K) on the device)."""
        def score_fn(T):
            core, R, S, O = self._operands_of(T)
            return score_candidates(core, R, S, O, subject_idx, relation_idx, candidates, tables=self._cached_tables(core, R))

        return score_fn

    def score_triples(self, subject_idx, relation_idx, object_idx):
        """``score_fn(T)`` giving the (B,) scores of the triples (h, r, t) (``ops.score_triples``)."""
        def score_fn(T):
            core, R, S, O = self._operands_of(T)
            return score_triples(core, R, S, O, subject_idx, relation_idx, object_idx, tables=self._cached_tables(core, R))

        return score_fn

    def _own(self, fn, *queries, tables=None, **kw):
        core, R, S, O = self._relation_operands()
        return fn(core, R, S, O, *queries, tables=self._cached_tables(core, R) if tables is None else tables, **kw)

    @torch.no_grad()
    def predict(self, subject_idx, relation_idx, k=10, flt=None, **kw):
        """The ``k`` most likely objects of each ``(subject, relation, ?)`` query, best first: ``(values, ids)``
        (``ops.topk_1vN``; ``flt``: a ``DeviceFilter`` whose known-true objects are left out).  In eval mode the
        relation tables are built once and reused, as by the scoring closure.  Keywords go to ``ops.topk_1vN``:
        ``matrix_free=True`` selects without storing any scores."""
        return self._own(topk_1vN, subject_idx, relation_idx, k, flt=flt, **kw)

    @torch.no_grad()
    def rank_objects(self, subject_idx, relation_idx, object_idx, flt=None, **kw):
        """Filtered rank of each ``(subject, relation, object)`` query against every entity (``ops.rank_1vN``;
        ``want_bce=True`` also returns the BCE row sums).  Relation tables as in ``predict``.  (``self.rank`` is the
        Tucker rank, as in the reference, hence the name.)"""
        return self._own(rank_1vN, subject_idx, relation_idx, object_idx, flt=flt, **kw)


class RelationQueriesMixin:
    """Relation prediction, (h, ?, t), for both model flavours: the model's own parameters (the flavour's
    ``_relation_operands()``) through ``ops.score_relations``."""

    def relation_logits(self, subject_idx, object_idx):
        """Logits ``(B, n_rel)`` of every relation for each ``(subject, ?, object)`` query, differentiable in the model's
        parameters (``ops.relation_logits``; the cached relation tables are not used): the input of a
        relation-classification loss such as ``ops.relation_ce_loss``."""
        from ..ops import relation_logits
        return relation_logits(*self._relation_operands(), subject_idx, object_idx)

    @torch.no_grad()
    def predict_relations(self, subject_idx, object_idx, k=10, flt=None):
        """The ``k`` most likely relations of each ``(subject, ?, object)`` query, best first: ``(values, ids)``
        (``ops.score_relations``, then ``evaluation.filtered_topk`` on the (B, n_rel) scores; ``flt``: a
        ``RelationFilter`` whose known-true relations are left out).  What the selection refuses (a ``k`` it does not
        take) is its own error."""
        from ..evaluation import filtered_topk
        from ..ops import score_relations
        P = score_relations(*self._relation_operands(), subject_idx, object_idx)
        if flt is None:
            return filtered_topk(P, k)
        return filtered_topk(P, k, flt, slots=flt.slots_of(subject_idx, object_idx))

    @torch.no_grad()
    def rank_relations(self, subject_idx, relation_idx, object_idx, flt=None, rank_type=None):
        """Filtered rank (B,) of ``relation_idx`` among all relations for each ``(subject, ?, object)`` query (``flt``: a
        ``RelationFilter``; the other known relations of the pair are set to 0).  ``rank_type``: None = the stable rule
        (int32, ``filtered_ranks``), or "optimistic" / "realistic" / "pessimistic" from the two tie counts
        (``ops.ranks_from_tie_counts``)."""
        from ..evaluation import _RowSlots, _check_tie_type, filtered_ranks, relation_tie_counts
        from ..ops import ranks_from_tie_counts, score_relations
        if rank_type is not None:
            _check_tie_type(rank_type)
        P = score_relations(*self._relation_operands(), subject_idx, object_idx)
        rel = torch.as_tensor(relation_idx).to(device=P.device, dtype=torch.int64).reshape(-1)
        slots = flt.slots_of(subject_idx, object_idx) if flt is not None else None
        if rank_type is None:
            if flt is None:
                return filtered_ranks(P, rel)
            return filtered_ranks(P, rel, _RowSlots(flt, slots), torch.arange(P.shape[0], device=P.device))
        greater, equal = relation_tie_counts(P, rel, flt, slots)
        return ranks_from_tie_counts(greater, equal, rank_type)
