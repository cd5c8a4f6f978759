"""Asymmetric R-TuckER (distinct subject / object embeddings) on the HIP scoring path.

Drop-in for ``src/model/asymmetric/R_TuckER.py`` of the reference: same constructor
(``R_TuckER((n_ent, n_rel), rank, **kwargs)``, train.py:203), same parameter names
and ``state_dict`` keys (``core``, ``S.weight``, ``R.weight``, ``O.weight``), same
``init`` recipe, same ``forward(subject_idx, relation_idx) -> score_fn(T)`` closure
protocol.  Only the closure body differs: one call into the C ABI instead of five
torch ops.
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
        self.S = nn.Embedding(n_ent, rank[1])
        self.R = nn.Embedding(n_rel, rank[0])
        self.O = nn.Embedding(n_ent, rank[2])
        self.core = nn.Parameter(torch.zeros(tuple(rank), dtype=torch.float32))
        self.rank = rank
        self._tables_reset()

    def init(self, state_dict=None):
        """Load a state dict, or Xavier-initialise and orthonormalise the factor
        columns by thin QR (reference: R_TuckER.py:27-39)."""
        self._tables_reset()
        if state_dict:
            self.load_state_dict(state_dict)
            return
        nn.init.xavier_uniform_(self.core)
        with torch.no_grad():
            for emb in (self.S, self.R, self.O):   # same RNG draw order as the reference
                nn.init.xavier_normal_(emb.weight)
            for emb in (self.S, self.O, self.R):
                emb.weight.data = torch.linalg.qr(emb.weight)[0]

    def forward(self, subject_idx, relation_idx):
        def score_fn(T):
            # sizes, dtype and device come from T, never from self.rank: during training
            # T is the doubled-rank tangent-space construct
            tables = self._cached_tables(T.core, T.factors[0])
            return score_1vN(T.core, T.factors[0], T.factors[1], T.factors[2], subject_idx, relation_idx, tables=tables)

        return score_fn

    def score_candidates(self, subject_idx, relation_idx, candidates):
        """``score_fn(T)`` giving the (B, K) scores of each query against its own candidate entities
        (``ops.score_candidates``; ``candidates`` int64 (B, K) on the device).  Like ``forward``, the sizes come from
        T, so it serves the doubled-rank T of training; in eval mode the relation tables are cached."""
        def score_fn(T):
            tables = self._cached_tables(T.core, T.factors[0])
            return score_candidates(T.core, T.factors[0], T.factors[1], T.factors[2], subject_idx, relation_idx, candidates, tables=tables)

        return score_fn

    def score_triples(self, subject_idx, relation_idx, object_idx):
        """``score_fn(T)`` giving the (B,) scores of the triples (h, r, t) (``ops.score_triples``)."""
        def score_fn(T):
            tables = self._cached_tables(T.core, T.factors[0])
            return score_triples(T.core, T.factors[0], T.factors[1], T.factors[2], subject_idx, relation_idx, object_idx, tables=tables)

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
        return topk_1vN(self.core, self.R.weight, self.S.weight, self.O.weight, subject_idx, relation_idx, k, flt=flt, tables=tables, **kw)

    @torch.no_grad()
    def rank_objects(self, subject_idx, relation_idx, object_idx, flt=None, **kw):
        """Filtered rank of each ``(subject, relation, object)`` query against every entity (``ops.rank_1vN``;
        ``want_bce=True`` also returns the BCE row sums).  Relation tables as in ``predict``.  (``self.rank`` is the
        Tucker rank, as in the reference, hence the name.)"""
        tables = kw.pop("tables", None)
        if tables is None:
            tables = self._cached_tables(self.core, self.R.weight)
        return rank_1vN(self.core, self.R.weight, self.S.weight, self.O.weight, subject_idx, relation_idx, object_idx, flt=flt,
                        tables=tables, **kw)
