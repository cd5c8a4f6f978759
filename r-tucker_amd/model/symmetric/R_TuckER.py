"""Symmetric (shared-factor) R-TuckER on the HIP scoring path.

Drop-in for ``src/model/symmetric/R_TuckER.py``: one entity matrix ``E`` serves as
subject gather source and as the 1-vs-all score operand; ``state_dict`` keys
``core``, ``E.weight``, ``R.weight``; ``score_fn`` reads ``T.regular_factors[0]``
and ``T.shared_factor`` (reference lines 40-44); the methods on top of the two hooks below are
``_tables.ObjectQueriesMixin``'s, shared with the asymmetric flavour.
"""
from __future__ import annotations

import torch
from torch import nn

from .._tables import ObjectQueriesMixin, RelationQueriesMixin, TablesCacheMixin


class R_TuckER(TablesCacheMixin, ObjectQueriesMixin, RelationQueriesMixin, nn.Module):
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

    def _operands_of(self, T):
        return T.core, T.regular_factors[0], T.shared_factor, T.shared_factor

    def _relation_operands(self):
        return self.core, self.R.weight, self.E.weight, self.E.weight
