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


class RelationQueriesMixin:
    """Relation prediction, (h, ?, t), for both model flavours: the model's own parameters through
    ``ops.score_relations`` (the symmetric model passes ``E`` as S and O)."""

    def _relation_operands(self):
        E = self.E.weight if hasattr(self, "E") else None
        return self.core, self.R.weight, (E if E is not None else self.S.weight), (E if E is not None else self.O.weight)

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
