"""Symmetric (shared-factor) R-TuckER on the HIP scoring path.

Drop-in for ``src/model/symmetric/R_TuckER.py``: one entity matrix ``E`` serves as
subject gather source and as the 1-vs-all score operand; ``state_dict`` keys
``core``, ``E.weight``, ``R.weight``; ``score_fn`` reads ``T.regular_factors[0]``
and ``T.shared_factor`` (reference lines 40-44).
"""
from __future__ import annotations

import torch
from torch import nn

from ...ops import rank_1vN, score_1vN, score_candidates, score_triples, topk_1vN
from .._tables import RelationQueriesMixin, TablesCacheMixin


class R_TuckER(TablesCacheMixin, RelationQueriesMixin, nn.Module):
    def __init__(self, data_count, rank=None, **kwargs):
        super().__init__()
        n_ent, n_rel = data_count
        self.E = nn.Embedding(n_ent, rank[1])
        self.R = nn.Embedding(n_rel, rank[0])
        self.core = nn.Parameter(torch.zeros(tuple(rank), dtype=torch.float32))
        self.rank = rank
        self._tables_reset()

    def init(self, state_dict=None):
        self._tables_reset()
        if state_dict:
            self.load_state_dict(state_dict)
            return
        nn.init.xavier_uniform_(self.core)
        with torch.no_grad():
            for emb in (self.E, self.R):
                nn.init.xavier_normal_(emb.weight)
            for emb in (self.E, self.R):
                emb.weight.data = torch.linalg.qr(emb.weight)[0]

    def forward(self, subject_idx, relation_idx):
        def score_fn(T):
            E = T.shared_factor
            tables = self._cached_tables(T.core, T.regular_factors[0])
            return score_1vN(T.core, T.regular_factors[0], E, E, subject_idx, relation_idx, tables=tables)

        return score_fn

    def score_candidates(self, subject_idx, relation_idx, candidates):
        """``score_fn(T)`` giving the (B, K) scores of each query against its own candidate entities
        (``ops.score_candidates``; ``candidates`` int64 (B, K) on the device).  Like ``forward``, the sizes come from
        T, so it serves the doubled-rank T of training; in eval mode the relation tables are cached.  ``E`` is passed as both S and O; autograd sums the two gradients."""
        def score_fn(T):
            E = T.shared_factor
            tables = self._cached_tables(T.core, T.regular_factors[0])
            return score_candidates(T.core, T.regular_factors[0], E, E, subject_idx, relation_idx, candidates, tables=tables)

        return score_fn

    def score_triples(self, subject_idx, relation_idx, object_idx):
        """``score_fn(T)`` giving the (B,) scores of the triples (h, r, t) (``ops.score_triples``)."""
        def score_fn(T):
            E = T.shared_factor
            tables = self._cached_tables(T.core, T.regular_factors[0])
            return score_triples(T.core, T.regular_factors[0], E, E, subject_idx, relation_idx, object_idx, tables=tables)

        return score_fn

    @torch.no_grad()
    def predict(self, subject_idx, relation_idx, k=10, flt=None, **kw):
        """The ``k`` most likely objects of each ``(subject, relation, ?)`` query, best first: ``(values, ids)``
        (``ops.topk_1vN``; ``flt``: a ``DeviceFilter`` whose known-true objects are left out).  In eval mode the
        relation tables are built once and reused, as by the scoring closure.  Keywords go to ``ops.topk_1vN``:
        ``matrix_free=True`` selects without storing any scores."""
        tables = kw.pop("tables", None)
        if tables is None:
            tables = self._cached_tables(self.core, self.R.weight)
        return topk_1vN(self.core, self.R.weight, self.E.weight, self.E.weight, subject_idx, relation_idx, k, flt=flt, tables=tables, **kw)

    @torch.no_grad()
    def rank_objects(self, subject_idx, relation_idx, object_idx, flt=None, **kw):
        """Filtered rank of each ``(subject, relation, object)`` query against every entity (``ops.rank_1vN``;
        ``want_bce=True`` also returns the BCE row sums).  Relation tables as in ``predict``.  (``self.rank`` is the
        Tucker rank, as in the reference, hence the name.)"""
        tables = kw.pop("tables", None)
        if tables is None:
            tables = self._cached_tables(self.core, self.R.weight)
        return rank_1vN(self.core, self.R.weight, self.E.weight, self.E.weight, subject_idx, relation_idx, object_idx, flt=flt,
                        tables=tables, **kw)
