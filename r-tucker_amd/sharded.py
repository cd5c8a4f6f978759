"""Entity-sharded 1-vs-all scoring across the GPUs of one node (one process per GPU).

The reference is single-device; this is the multi-GPU form BASELINE.json's north_star
asks for: the entity matrix O (asymmetric) / E (symmetric) is partitioned into
contiguous row blocks, one per rank; every rank scores the whole (h, r) batch
against ITS block with the local HIP kernels -- score columns are independent per
entity, ``Z[:, J_p] = v . O[J_p, :]^T`` -- and the per-shard score blocks are
exchanged with ONE collective, an all-gather (RCCL over xGMI when the process group
is "nccl").  The core tensor, the relation matrix and the subject-lookup matrix stay
replicated (they are small next to the B x N score block).

Layout.  Shards are padded to equal size ``n_loc = ceil(N / P)``; the all-gather
concatenates along dim 0, so the gathered buffer is ``(P, B, n_loc)`` with rank p's
block in slot p.  ``scores_rowmajor`` turns it into the reference's ``(B, N)``
(one strided copy); consumers that can work shard-wise should use the gathered
buffer directly (``view_BPn``) and skip that copy.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def _identity(t):
    return t


class EntityShards:
    """Row partition of ``n_ent`` entities over ``world`` ranks."""

    def __init__(self, n_ent: int, world: int):
        if n_ent <= 0 or world <= 0:
            raise ValueError("n_ent and world must be positive")
        self.n_ent, self.world = int(n_ent), int(world)
        self.n_loc = -(-self.n_ent // self.world)   # ceil: every shard padded to this many rows

    def bounds(self, rank: int):
        lo = min(rank * self.n_loc, self.n_ent)
        return lo, min(lo + self.n_loc, self.n_ent)

    def take(self, full: torch.Tensor, rank: int) -> torch.Tensor:
        """This rank's (n_loc, c) block of a full (N, c) matrix, zero-padded at the end."""
        lo, hi = self.bounds(rank)
        out = torch.zeros((self.n_loc,) + tuple(full.shape[1:]), dtype=full.dtype, device=full.device)
        out[: hi - lo] = full[lo:hi]
        return out


class ShardedEntityScorer:
    """``score(...)`` = the reference's ``score_fn`` with O row-sharded over a process group.

    ``local_score(core, R, S, O_loc, h, r, out=...)`` computes the (B, n_loc) block; the
    default is the HIP path (``ops.score_1vN_into``).  Tests inject CPU functions to
    exercise the sharding / gather logic under the gloo backend.

    Stage 1 (the query vectors) is cheap next to a shard's score block when the relation rank is small
    (WN18RR: a = 10) and is then simply replicated.  For a large relation rank it is as expensive as the
    whole score shard (C5: 1.1 TFLOP), so with ``stage1="split"`` (the ``"auto"`` choice
    for a > 32) every rank contracts only its ``ceil(B / P)`` slice of the batch, the ``(B, c)`` fp32
    vectors are exchanged with one small all-gather (16 MB at C5) and each rank packs them for its score
    kernel.  The rows are computed by the same kernels either way: bit-identical scores.
    ``stage1="relation"`` (needs the prebuilt relation ``tables``) splits by RELATION instead: rank p contracts the
    queries whose relation id is congruent to p modulo P and streams only those relations' tables -- at C5 (8192
    queries over 1000 relations of 1 MB each) a batch slice of 1024 queries still touches ~640 tables, the
    relation split 125 -- and one all-reduce(SUM) of the zero-initialised ``(B, c)`` buffers completes the vectors
    (every row is non-zero on exactly one rank: the sum is exact, the scores bit-identical again).

    ``score_dtype=torch.bfloat16`` (bf16 operands): the local kernel writes bf16 scores, which halves the
    score exchange.
    """

    def __init__(self, n_ent: int, group=None, local_score=None, stage1="auto", score_dtype=torch.float32,
                 query_vectors_fn=None, score_from_v_fn=None, collective="torch"):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.shards = EntityShards(n_ent, self.world)
        if local_score is None:
            from .ops import score_1vN_into
            local_score = score_1vN_into
        self.local_score = local_score
        if stage1 not in ("auto", "replicated", "split", "relation"):
            raise ValueError("stage1 must be auto | replicated | split | relation")
        self.stage1 = stage1
        self.score_dtype = score_dtype
        self.query_vectors_fn = query_vectors_fn
        self.score_from_v_fn = score_from_v_fn
        self._gathered = None
        self._v_all = None
        self._v_rel = None
        self.query_vectors_part_fn = None       # tests inject a CPU function for stage1="relation"
        self.pack_fn = None                     # tests inject a CPU stand-in for ops.pack_query_vectors (rank_1vN)
        # the score exchange: "torch" = torch.distributed's all_gather_into_tensor on the process group (RCCL when
        # the backend is "nccl"); "abi" = the C ABI's own communicator (rtk_comm_init / rtk_allgather_scores:
        # RCCL bound by the library itself -- the path a non-Python host takes; torch.distributed only carries the
        # 128-byte unique id from rank 0 to the others, once)
        if collective not in ("torch", "abi"):
            raise ValueError("collective must be torch | abi")
        self.collective = collective
        self._comm = None

    def _abi_comm(self, device):
        if self._comm is None:
            import ctypes as C
            from . import _lib
            lib = _lib.load()
            ident = torch.zeros(128, dtype=torch.uint8)
            if self.rank == 0:
                buf = (C.c_ubyte * 128)()
                _lib.check(lib.rtk_comm_unique_id(buf), "rtk_comm_unique_id")
                ident = torch.tensor(list(buf), dtype=torch.uint8)
            if self.world > 1:
                backend = dist.get_backend(self.group)
                carrier = ident.to(device) if backend == "nccl" else ident
                dist.broadcast(carrier, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
                ident = carrier.cpu()
            raw = bytes(ident.tolist())
            comm = C.c_void_p()
            with torch.cuda.device(device):
                _lib.check(lib.rtk_comm_init(self.rank, self.world, raw, C.byref(comm)), "rtk_comm_init")
            self._comm = comm
        return self._comm

    def close(self):
        """Destroy the C-ABI communicator, if one was made."""
        if self._comm is not None:
            from . import _lib
            _lib.check(_lib.load().rtk_comm_destroy(self._comm), "rtk_comm_destroy")
            self._comm = None

    def _exchange(self, g: torch.Tensor):
        """Complete the (P, B, pitch) buffer in place: slot p comes from rank p."""
        if self.collective == "abi":
            from . import _lib
            with torch.cuda.device(g.device):
                _lib.check(_lib.load().rtk_allgather_scores(self._abi_comm(g.device), g.data_ptr(),
                                                            g[0].numel() * g.element_size(),
                                                            torch.cuda.current_stream(g.device).cuda_stream),
                           "rtk_allgather_scores")
        elif self.world > 1:
            # in-place all-gather of the padded storage: input is the rank-th slice of the output buffer
            dist.all_gather_into_tensor(g.view(-1), g[self.rank].view(-1), group=self.group)

    def local_block(self, full_entity_matrix: torch.Tensor) -> torch.Tensor:
        return self.shards.take(full_entity_matrix, self.rank)

    def _buffer(self, B, device, dtype):
        # rows start on 128-byte boundaries (ops.alloc_scores): the storage is (P, B, pitch)
        from .ops import _row_pitch
        need = (self.world, B, _row_pitch(self.shards.n_loc, dtype))
        g = self._gathered
        if g is None or tuple(g.shape) != need or g.device != device or g.dtype != dtype:
            g = torch.empty(need, dtype=dtype, device=device)
            self._gathered = g
        return g

    def _real_rows(self):
        """``(lo, n_valid)``: this rank's rows of ``O_loc`` that are entities, ``[lo, lo + n_valid)`` of the entity
        matrix.  The last shard's padding rows are not entities, and a rank that lies wholly past ``n_ent`` has none."""
        lo, hi = self.shards.bounds(self.rank)
        return lo, hi - lo

    def _all_reduce(self, op):
        """``fn(t)``, the all-reduce of ``t`` in place over the group; None at world size 1, where nothing is exchanged."""
        if self.world == 1:
            return None
        return lambda t: dist.all_reduce(t, op=op, group=self.group)

    @property
    def row_sum(self):
        """``fn(t) -> t``: the SUM all-reduce of a small tensor in place over this scorer's group (the identity at world
        size 1) -- the entry of ``Tucker.row_sum`` for a factor whose rows are sharded as ``local_block`` shards them."""
        if self.world == 1:
            return _identity

        def fn(t):
            c = t if t.is_contiguous() else t.contiguous()
            dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.group)
            return t if c is t else t.copy_(c)
        return fn

    def tucker(self, core, R, S, O_loc):
        """The point ``core x (R, S, O)`` of the asymmetric model with O row-sharded: a ``Tucker`` on this rank's block
        ``O_loc`` whose Riemannian operations (gradient, projection, norms, retraction: ``riemannian.py``, ``optim.py``)
        complete every sum over O's rows with one small all-reduce.  Core, R and S are replicated and come out of a step
        identical on every rank; the padding rows of the last shard stay zero."""
        from .tucker import Tucker
        return Tucker(core, [R, S, O_loc], row_sum=[None, None, self.row_sum])

    def _loss_steps(self, default, dtype, **injected):
        """The steps of a block loss: the class ``default`` of ``ops``, or, when a test injects CPU functions (the
        ``injected`` steps by name, ``query_vectors_fn`` / ``pack_fn`` for stage 1), a namespace that has them in the
        default steps' places and checks no operands."""
        if not any(injected.values()) and self.query_vectors_fn is None:
            return default
        from types import SimpleNamespace
        from .ops import pack_query_vectors

        def queries(core, R, S, h, r):
            v = self.query_vectors_fn(core, R, S, h, r)
            return v, (self.pack_fn or pack_query_vectors)(v, dtype)

        return SimpleNamespace(
            operands=lambda c_, R_, S_, O_, h, r, col0, n, who: (c_, R_, S_, O_, h.view(-1), r.view(-1)),
            queries=queries if self.query_vectors_fn is not None else default.queries,
            **{name: fn or getattr(default, name) for name, fn in injected.items()})

    def _split_stage1(self, core) -> bool:
        if self.world == 1 or self.stage1 == "replicated":
            return False
        return self.stage1 in ("split", "relation") or core.shape[0] > 32

    def query_vectors_by_relation(self, core, R, S, subject_idx, relation_idx, tables) -> torch.Tensor:
        """``(B, c)`` fp32 query vectors with stage 1 split over the ranks by relation id (``stage1="relation"``)."""
        B = int(subject_idx.numel())
        c = core.shape[2]
        v = self._v_rel
        if v is None or tuple(v.shape) != (B, c) or v.device != core.device:
            v = self._v_rel = torch.empty((B, c), dtype=torch.float32, device=core.device)
        v.zero_()
        fn = self.query_vectors_part_fn
        if fn is None:
            from .ops import query_vectors_part as fn
        fn(core, R, S, subject_idx.view(-1), relation_idx.view(-1), tables, self.rank, self.world, v)
        if self.world > 1:
            dist.all_reduce(v, op=dist.ReduceOp.SUM, group=self.group)
        return v

    def query_vectors_split(self, core, R, S, subject_idx, relation_idx, **kw) -> torch.Tensor:
        """``(B, c)`` fp32 query vectors with the batch split over the ranks: this rank contracts queries
        ``[rank * B_loc, (rank + 1) * B_loc)``, one all-gather of ``B_loc x c`` floats assembles the rest."""
        B = int(subject_idx.numel())
        c = core.shape[2]
        B_loc = -(-B // self.world)
        lo, hi = min(self.rank * B_loc, B), min((self.rank + 1) * B_loc, B)
        va = self._v_all
        if va is None or tuple(va.shape) != (self.world * B_loc, c) or va.device != core.device:
            va = self._v_all = torch.zeros((self.world * B_loc, c), dtype=torch.float32, device=core.device)
        fn = self.query_vectors_fn
        if fn is None:
            from .ops import query_vectors as fn
        mine = va[self.rank * B_loc:(self.rank + 1) * B_loc]
        if hi > lo:
            mine[: hi - lo].copy_(fn(core, R, S, subject_idx.view(-1)[lo:hi], relation_idx.view(-1)[lo:hi], **kw))
        dist.all_gather_into_tensor(va.view(-1), mine.reshape(-1), group=self.group)
        return va[:B]

    def _score_local(self, core, R, S, O_loc, subject_idx, relation_idx, mine, tables=None, **kw):
        if not self._split_stage1(core):
            if tables is not None:
                kw = dict(kw, tables=tables)
            self.local_score(core, R, S, O_loc, subject_idx, relation_idx, out=mine, **kw)
            return
        qkw = {"tables": tables} if tables is not None else {}
        if self.stage1 == "relation" and tables is not None:
            v = self.query_vectors_by_relation(core, R, S, subject_idx, relation_idx, tables)
        else:
            v = self.query_vectors_split(core, R, S, subject_idx, relation_idx, **qkw)
        if self.score_from_v_fn is not None:
            self.score_from_v_fn(v, O_loc, out=mine, **kw)
        else:
            from .ops import pack_query_vectors, score_packed_into
            score_packed_into(pack_query_vectors(v, O_loc.dtype), v.shape[0], O_loc, mine, **kw)

    def score_gathered(self, core, R, S, O_loc, subject_idx, relation_idx, tables=None, **kw) -> torch.Tensor:
        """All ranks' score blocks, ``(P, B, n_loc)``; slot p = rank p's entities.
        Columns past the real entity count in the last shard are padding (sigmoid(0) = 0.5)."""
        B = int(subject_idx.numel())
        g = self._buffer(B, core.device, self.score_dtype)
        n_loc = self.shards.n_loc
        mine = g[self.rank][:, :n_loc]                        # (B, n_loc) view: the kernel writes in place
        self._score_local(core, R, S, O_loc, subject_idx, relation_idx, mine, tables=tables, **kw)
        self._exchange(g)
        return g[:, :, :n_loc]

    def view_BPn(self, gathered: torch.Tensor) -> torch.Tensor:
        """(B, P, n_loc) view of the gathered buffer: [d, p, i] = score of entity p*n_loc + i."""
        return gathered.permute(1, 0, 2)

    def scores_rowmajor(self, gathered: torch.Tensor) -> torch.Tensor:
        """The reference's (B, N) layout (copies)."""
        B = gathered.shape[1]
        return self.view_BPn(gathered).reshape(B, self.world * self.shards.n_loc)[:, : self.shards.n_ent].contiguous()

    def score(self, core, R, S, O_loc, subject_idx, relation_idx, **kw) -> torch.Tensor:
        return self.scores_rowmajor(self.score_gathered(core, R, S, O_loc, subject_idx, relation_idx, **kw))

    # ---- ranking without the gather ("better than gather") -------------------
    def filtered_ranks(self, core, R, S, O_loc, subject_idx, relation_idx, object_idx, flt=None, item_ids=None,
                       want_bce=False, target_scores_fn=None, rank_counts_fn=None, **kw):
        """Filtered rank of ``object_idx`` (global entity ids) for every query, with the entity
        matrix row-sharded and NO exchange of scores: each rank scores its block, the target
        scores are completed by one all-reduce(MAX) of B floats, the per-block counts by one
        all-reduce(SUM) of B int32 (+ B doubles for the BCE sums).  Same numbers as
        ``evaluation.filtered_ranks`` on the gathered matrix (the count is a sum over columns).

        ``target_scores_fn`` / ``rank_counts_fn`` default to the HIP kernels
        (``evaluation.target_scores_block`` / ``rank_counts_block``); tests inject CPU functions."""
        if target_scores_fn is None or rank_counts_fn is None:
            from .evaluation import rank_counts_block, target_scores_block
            target_scores_fn = target_scores_fn or target_scores_block
            rank_counts_fn = rank_counts_fn or rank_counts_block
        B = int(subject_idx.numel())
        lo, n_valid = self._real_rows()
        g = self._buffer(B, core.device, torch.float32)      # the ranking kernels read fp32 scores
        mine = g[self.rank][:, :self.shards.n_loc]
        self._score_local(core, R, S, O_loc, subject_idx, relation_idx, mine, **kw)
        block = mine[:, :n_valid] if n_valid > 0 else None
        pt = (target_scores_fn(block, object_idx, lo) if block is not None
              else torch.full((B,), float("-inf"), dtype=torch.float32, device=core.device))
        if self.world > 1:
            dist.all_reduce(pt, op=dist.ReduceOp.MAX, group=self.group)
        res = rank_counts_fn(block, object_idx, lo, pt, flt, item_ids, want_bce) if block is not None else None
        return self._ranks_from_counts(res, B, core.device, want_bce)

    def _ranks_from_counts(self, res, B, device, want_bce):
        """Ranks from the block's ``counts`` or ``(counts, bce)`` (None: a rank without rows, which counts nothing): one
        all-reduce(SUM) of B int32 (+ B doubles for the BCE sums), rank = count + 1."""
        if res is None:
            res = torch.zeros(B, dtype=torch.int32, device=device)
            res = (res, torch.zeros(B, dtype=torch.float64, device=device)) if want_bce else res
        counts, bce = res if want_bce else (res, None)
        if self.world > 1:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
            if want_bce:
                dist.all_reduce(bce, op=dist.ReduceOp.SUM, group=self.group)
        ranks = counts + 1
        return (ranks, bce) if want_bce else ranks

    # ---- ranking without the gather and without the score block --------------------------------
    def _packed_queries(self, core, R, S, dtype, subject_idx, relation_idx, tables):
        """Packed query planes of the batch, stage 1 by the scorer's policy (replicated, "split", "relation")."""
        qkw = {"tables": tables} if tables is not None else {}
        if self._split_stage1(core):
            if self.stage1 == "relation" and tables is not None:
                v = self.query_vectors_by_relation(core, R, S, subject_idx, relation_idx, tables)
            else:
                v = self.query_vectors_split(core, R, S, subject_idx, relation_idx, **qkw)
        elif self.query_vectors_fn is not None:
            v = self.query_vectors_fn(core, R, S, subject_idx.view(-1), relation_idx.view(-1), **qkw)
        else:
            from .ops import query_vectors
            return query_vectors(core, R, S, subject_idx, relation_idx, packed=True, **qkw)[1]
        pack = self.pack_fn
        if pack is None:
            from .ops import pack_query_vectors as pack
        return pack(v, dtype)

    def _rank_targets(self, core, R, S, O_loc, subject_idx, relation_idx, object_idx, flt, tables, sigmoid_mode, targets_fn):
        """The first step of ``rank_1vN`` and ``rank_ties_1vN`` -> ``(qp, rows, lo, slots, pt)``: the packed query planes,
        this rank's real rows of ``O_loc`` (None for a rank without rows) and their first global row, the queries' filter
        slots, and the target scores completed by one all-reduce(MAX) of B floats."""
        if targets_fn is None:
            from .ops import rank_targets_block as targets_fn
        B = int(subject_idx.numel())
        lo, n_valid = self._real_rows()
        slots = flt.slots_of(subject_idx, relation_idx) if flt is not None else None
        qp = self._packed_queries(core, R, S, O_loc.dtype, subject_idx, relation_idx, tables)
        rows = O_loc[:n_valid] if n_valid > 0 else None
        pt = (targets_fn(qp, B, rows, lo, self.shards.n_ent, object_idx, sigmoid_mode=sigmoid_mode) if rows is not None
              else torch.full((B,), float("-inf"), dtype=torch.float32, device=core.device))
        if self.world > 1:
            dist.all_reduce(pt, op=dist.ReduceOp.MAX, group=self.group)
        return qp, rows, lo, slots, pt

    def rank_1vN(self, core, R, S, O_loc, subject_idx, relation_idx, object_idx, flt=None, want_bce=False, tables=None,
                 sigmoid_mode=None, targets_fn=None, counts_fn=None):
        """``filtered_ranks`` without the (B, n_loc) score block: stage 1 once into packed query planes, the target
        scores of this rank's rows (``ops.rank_targets_block``) completed by one all-reduce(MAX) of B floats, the
        block's counts (``ops.rank_counts_block_1vN``: scored and counted in one entity-stationary pass) by one
        all-reduce(SUM) of B int32 (+ B doubles for the BCE sums); rank = count + 1.  ``object_idx`` and the filter
        hold global entity ids.  Equals ``ops.rank_1vN`` on the whole entity matrix exactly.

        ``targets_fn`` / ``counts_fn`` take the arguments of the two ``ops`` functions; tests inject CPU functions
        (with ``query_vectors_fn`` / ``pack_fn`` for stage 1)."""
        if counts_fn is None:
            from .ops import rank_counts_block_1vN as counts_fn
        B = int(subject_idx.numel())
        qp, rows, lo, slots, pt = self._rank_targets(core, R, S, O_loc, subject_idx, relation_idx, object_idx, flt, tables,
                                                     sigmoid_mode, targets_fn)
        res = counts_fn(qp, B, rows, lo, self.shards.n_ent, pt, object_idx, flt=flt, slots=slots, want_bce=want_bce,
                        sigmoid_mode=sigmoid_mode) if rows is not None else None
        return self._ranks_from_counts(res, B, core.device, want_bce)

    def rank_ties_1vN(self, core, R, S, O_loc, subject_idx, relation_idx, object_idx, flt=None, tables=None,
                      sigmoid_mode=None, targets_fn=None, tie_counts_fn=None):
        """The tie counts ``(greater, equal)`` (int32, B) of ``ops.rank_ties_1vN`` on entity shards, without the
        (B, n_loc) score block: ``rank_1vN``'s steps with ``ops.rank_tie_counts_block_1vN`` as the second -- one
        all-reduce(MAX) of B floats for the target scores, one all-reduce(SUM) of a (2, B) int32 tensor for both
        counts.  Equals ``ops.rank_ties_1vN`` on the whole entity matrix exactly; a rank without rows contributes
        zeros and still takes part in both all-reduces.

        ``targets_fn`` / ``tie_counts_fn`` take the arguments of the two ``ops`` functions; tests inject CPU functions
        (with ``query_vectors_fn`` / ``pack_fn`` for stage 1)."""
        if tie_counts_fn is None:
            from .ops import rank_tie_counts_block_1vN as tie_counts_fn
        B = int(subject_idx.numel())
        qp, rows, lo, slots, pt = self._rank_targets(core, R, S, O_loc, subject_idx, relation_idx, object_idx, flt, tables,
                                                     sigmoid_mode, targets_fn)
        both = torch.zeros((2, B), dtype=torch.int32, device=core.device)
        if rows is not None:
            greater, equal = tie_counts_fn(qp, B, rows, lo, self.shards.n_ent, pt, object_idx, flt=flt, slots=slots,
                                           sigmoid_mode=sigmoid_mode)
            both[0], both[1] = greater, equal
        if self.world > 1:
            dist.all_reduce(both, op=dist.ReduceOp.SUM, group=self.group)
        return both[0], both[1]

    # ---- the training loss without the gather and without the score block ----------------------
    def bce_loss_1vN(self, core, R, S, O_loc, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0,
                     sigmoid_mode=None, max_pos=None, rows_fn=None, grad_o_fn=None, stage1_bwd_fn=None):
        """The 1-vs-all BCE training loss with the entity matrix row-sharded and nothing of size B x n_loc allocated
        (``ops.bce_loss_block_1vN`` on this rank's REAL rows, ``col0 = rank * n_loc``; ``flt`` holds global entity
        ids).  The loss is a sum over entities: the forward completes the B float64 loss rows with one
        all-reduce(SUM) and returns the whole loss, equal on every rank.  The backward completes dv (B x c floats)
        with one all-reduce(SUM) before the stage-1 backward, so ``core.grad``, ``R.grad`` and ``S.grad`` are complete
        and identical on every rank (do not average them again); ``O_loc.grad`` is this rank's rows of the gradient
        of O and needs no exchange.  The last shard's zero padding rows are not entities: they add neither loss nor
        smoothing terms and their gradient is 0.  A rank without rows contributes zeros and still takes part in both
        all-reduces.  Without a process group (world size 1) this is ``ops.bce_loss_1vN(..., matrix_free=True)`` bit
        for bit.  bfloat16 operands (all four; ``c <= 512``, ``c % 8 == 0``) run the same steps on
        ``rtk_bce_stream_*_part_bf16`` as in ``ops.bce_loss_block_1vN``, which the call equals bit for bit at world
        size 1; the gradients come back in bf16 and the all-reduces (B doubles, B x c floats) are unchanged.

        Stage 1 and its backward stay replicated: every rank computes all B query vectors from the replicated core,
        R and S (the scorer's ``stage1`` policy does not apply here).

        ``rows_fn`` / ``grad_o_fn`` / ``stage1_bwd_fn`` take the arguments of ``ops._HipBlockLossAnyDtype.rows`` / ``grad_o``
        / ``stage1_backward``; tests inject CPU functions (with ``query_vectors_fn`` / ``pack_fn`` for stage 1)."""
        from . import ops
        lo, n_valid = self._real_rows()
        steps = self._loss_steps(ops._HipBlockLossAnyDtype, O_loc.dtype, rows=rows_fn, grad_o=grad_o_fn,
                                 stage1_backward=stage1_bwd_fn)
        return ops._block_loss(steps, core, R, S, O_loc[:n_valid], lo, self.shards.n_ent, subject_idx, relation_idx, flt,
                               item_ids, label_smoothing, sigmoid_mode, max_pos, self._all_reduce(dist.ReduceOp.SUM))

    def ce_loss_1vN(self, core, R, S, O_loc, subject_idx, relation_idx, flt, item_ids, label_smoothing=0.0, max_pos=None,
                    partials_fn=None, grad_fn=None, stage1_bwd_fn=None):
        """The 1-vs-all softmax cross-entropy training loss with the entity matrix row-sharded and nothing of size
        B x n_loc allocated (``ops.ce_loss_block_1vN`` on this rank's REAL rows, ``col0 = rank * n_loc``; ``flt`` holds
        global entity ids).  The row's log-sum-exp couples the shards, so the forward has two exchanges: one
        all-reduce(MAX) of the B float32 block maxima, then one all-reduce(SUM) of a (2, B) float64 tensor (the blocks'
        sums of exponentials at the common maximum, and their linear parts); the loss is complete and equal on every
        rank.  The backward runs on the global lse and completes dv (B x c floats) with one all-reduce(SUM) before the
        stage-1 backward, so ``core.grad``, ``R.grad`` and ``S.grad`` are complete and identical on every rank (do not
        average them again); ``O_loc.grad`` is this rank's rows of the gradient of O and needs no exchange.  The last
        shard's zero padding rows are not entities: they enter neither the log-sum-exp nor the smoothing term and
        their gradient is 0.  A rank without rows contributes ``m = -inf, s = 0, lin = 0`` and zero dv and still takes
        part in all three exchanges.  Every world size runs the same block loss; without a process group (world size 1)
        nothing is exchanged and the call is the one ``ops.ce_loss_1vN(..., matrix_free=True)`` makes: the whole range as
        one block.

        Stage 1 and its backward stay replicated, as in ``bce_loss_1vN``.

        ``partials_fn`` / ``grad_fn`` / ``stage1_bwd_fn`` take the arguments of ``ops._HipCeBlockLoss.partials`` /
        ``grad`` / ``stage1_backward``; tests inject CPU functions (with ``query_vectors_fn`` / ``pack_fn`` for
        stage 1)."""
        from . import ops
        lo, n_valid = self._real_rows()
        steps = self._loss_steps(ops._HipCeBlockLoss, O_loc.dtype, partials=partials_fn, grad=grad_fn,
                                 stage1_backward=stage1_bwd_fn)
        return ops._ce_block_loss(steps, core, R, S, O_loc[:n_valid], lo, self.shards.n_ent, subject_idx, relation_idx, flt,
                                  item_ids, label_smoothing, max_pos, self._all_reduce(dist.ReduceOp.SUM),
                                  self._all_reduce(dist.ReduceOp.MAX), None, who="ShardedEntityScorer.ce_loss_1vN")

    # ---- top-k without the gather ----------------------------------------------------------
    def topk(self, core, R, S, O_loc, subject_idx, relation_idx, k, flt=None, slots=None, keep_idx=None,
             local_topk_fn=None, merge_fn=None, matrix_free=False, **kw):
        """Filtered top-k objects (``(values, ids)``, (B, k), global entity ids, best first) with the entity matrix
        row-sharded and NO exchange of scores: each rank scores its block and selects its top k over its real
        columns (``col0 = rank * n_loc``; the last shard's padding rows are never candidates), the (B, k) lists are
        all-gathered -- B k 12 bytes per rank instead of B N 4 -- and merged.  Same result as ``filtered_topk`` on the
        gathered matrix.  ``slots`` default to ``flt.slots_of(subject_idx, relation_idx)``.

        ``local_topk_fn(P_block, k, col0, flt, slots, keep_idx)`` / ``merge_fn(values, ids, k)`` default to the HIP
        select (``evaluation.filtered_topk``, plain and merge mode); tests inject CPU functions.

        ``matrix_free=True``: the (B, n_loc) score block is not formed either.  Stage 1 goes into packed query planes
        and the local step is ``ops.topk_block_1vN`` on this rank's real rows (``local_topk_fn`` then takes ITS
        arguments: ``(qp, B, O_rows, col0, n_ent, k, flt=, slots=, keep_idx=, sigmoid_mode=)``); all-gather and merge
        are the same.  Equals ``ops.topk_1vN(..., matrix_free=True)`` on the whole entity matrix exactly.  Keywords:
        ``tables``, ``sigmoid_mode``."""
        if matrix_free:
            return self._topk_matrix_free(core, R, S, O_loc, subject_idx, relation_idx, k, flt, slots, keep_idx,
                                          local_topk_fn, merge_fn, **kw)
        if local_topk_fn is None or merge_fn is None:
            from .evaluation import filtered_topk
            local_topk_fn = local_topk_fn or (lambda P, k_, col0, flt_, slots_, keep_: filtered_topk(
                P, k_, flt_, keep_idx=keep_, slots=slots_, col0=col0))
            merge_fn = merge_fn or (lambda v, i, k_: filtered_topk(v, k_, ids=i))
        B = int(subject_idx.numel())
        lo, n_valid = self._real_rows()
        if slots is None and flt is not None:
            slots = flt.slots_of(subject_idx, relation_idx)
        g = self._buffer(B, core.device, self.score_dtype)
        mine = g[self.rank][:, :self.shards.n_loc]
        self._score_local(core, R, S, O_loc, subject_idx, relation_idx, mine, **kw)
        values, ids = local_topk_fn(mine[:, :n_valid], k, lo, flt, slots, keep_idx)
        return self._merge_topk(values, ids, B, k, merge_fn)

    def _topk_matrix_free(self, core, R, S, O_loc, subject_idx, relation_idx, k, flt, slots, keep_idx, local_topk_fn,
                          merge_fn, tables=None, sigmoid_mode=None):
        if local_topk_fn is None:
            from .ops import topk_block_1vN as local_topk_fn
        if merge_fn is None:
            from .evaluation import filtered_topk
            merge_fn = lambda v, i, k_: filtered_topk(v, k_, ids=i)                      # noqa: E731
        B = int(subject_idx.numel())
        lo, n_valid = self._real_rows()
        if slots is None and flt is not None:
            slots = flt.slots_of(subject_idx, relation_idx)
        qp = self._packed_queries(core, R, S, O_loc.dtype, subject_idx, relation_idx, tables)
        if n_valid > 0:
            values, ids = local_topk_fn(qp, B, O_loc[:n_valid], lo, self.shards.n_ent, k, flt=flt, slots=slots,
                                        keep_idx=keep_idx, sigmoid_mode=sigmoid_mode)
        else:                                                     # a rank without rows: an empty list
            values = torch.full((B, k), float("-inf"), dtype=torch.float32, device=core.device)
            ids = torch.full((B, k), -1, dtype=torch.int64, device=core.device)
        return self._merge_topk(values, ids, B, k, merge_fn)

    def _merge_topk(self, values, ids, B, k, merge_fn):
        """The ranks' (B, k) lists all-gathered and merged (one rank: its list is the result)."""
        if self.world == 1:
            return values, ids
        gv = torch.empty((self.world, B, k), dtype=values.dtype, device=values.device)
        gi = torch.empty((self.world, B, k), dtype=ids.dtype, device=ids.device)
        dist.all_gather_into_tensor(gv.view(-1), values.contiguous().view(-1), group=self.group)
        dist.all_gather_into_tensor(gi.view(-1), ids.contiguous().view(-1), group=self.group)
        # rank order = ascending id ranges: tied values stay in ascending id order for the merge
        return merge_fn(gv.permute(1, 0, 2).reshape(B, self.world * k), gi.permute(1, 0, 2).reshape(B, self.world * k), k)
