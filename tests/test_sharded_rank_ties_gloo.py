"""``ShardedEntityScorer.rank_ties_1vN`` (the tie counts on entity shards without the score block) under the gloo
backend, world_size 2, on CPU, in the manner of tests/test_sharded_rank_gloo.py: the two block steps are injected as CPU
functions that restate ``rtk_score_rank_targets_*`` / ``rtk_score_rank_tie_counts_*`` on plain query vectors, so the
host logic -- stage 1 once, ownership by global id, the padding rows of the last shard, the MAX all-reduce of B floats
and the SUM all-reduce of the (2, B) counts -- runs without a GPU.  The result must equal the numpy model
(tests/tie_model.py) on the full matrix, and bracket the oracle's stable rank."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gen
import tie_model
from oracle import score_oracle as orc


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _Flt:
    """The CSR arrays of evaluation.DeviceFilter on the CPU; one list per query."""
    def __init__(self, pair_ptr, pair_obj):
        self.pair_ptr, self.pair_obj = pair_ptr, pair_obj

    def slots_of(self, h, r):
        return torch.arange(h.numel())


def _scores(v, O):
    """float64 products rounded to float32: a score does not depend on which rows are scored with it."""
    return torch.sigmoid((v.double() @ O.double().T).float())


def _cpu_targets(v, B, O_loc, col0, n_ent, obj, sigmoid_mode=None):
    P = _scores(v, O_loc)
    j = obj - col0
    own = (j >= 0) & (j < O_loc.shape[0])
    pt = torch.full((B,), float("-inf"))
    pt[own] = P[own.nonzero().view(-1), j[own]]
    return pt


def _cpu_tie_counts(v, B, O_loc, col0, n_ent, pt, obj, flt=None, slots=None, sigmoid_mode=None):
    lists = None
    if flt is not None:
        lists = [flt.pair_obj[flt.pair_ptr[int(s)]:flt.pair_ptr[int(s) + 1]].tolist() if int(s) >= 0 else None
                 for s in slots]
    gt, eq, _ = tie_model.tie_counts(_scores(v, O_loc).numpy(), obj.numpy(), known=lists, col0=col0, pt=pt.numpy())
    return torch.from_numpy(gt).to(torch.int32), torch.from_numpy(eq).to(torch.int32)


def _worker(rank, world, port, n_ent, far_targets, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from r_tucker_amd.sharded import ShardedEntityScorer
        n_rel, B, rank3 = 5, 24, (3, 8, 8)
        core, R, S, O = [torch.from_numpy(x) for x in gen.make_params(n_ent, n_rel, rank3, 9)]
        O = O[torch.arange(n_ent) % 13]               # every row 4 to 8 times, in both shards -> exact ties
        h, r = [torch.from_numpy(x) for x in gen.make_queries(n_ent, n_rel, B, 9)]
        rng = np.random.default_rng(9)
        # far_targets: every queried object lies in rank 0's shard, so rank 1 owns no target at all
        obj = torch.from_numpy(rng.integers(0, n_ent // 2 if far_targets else n_ent, B))
        lists = [sorted(set([int(obj[d])] + rng.integers(0, n_ent, rng.integers(0, 6)).tolist())) for d in range(B)]
        ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64)
        flt = _Flt(ptr, torch.tensor([x for l in lists for x in l], dtype=torch.int64))
        calls = []

        def qv(core_, R_, S_, hh, rr, **kw):
            calls.append(int(hh.numel()))
            return orc.query_vectors_ref(core_, R_, S_, hh, rr)

        sc = ShardedEntityScorer(n_ent, query_vectors_fn=qv)
        sc.pack_fn = lambda v, dtype: v
        O_loc = sc.local_block(O)
        padded = O_loc.shape[0] * world > n_ent           # the last shard carries rows that are not entities
        gt, eq = sc.rank_ties_1vN(core, R, S, O_loc, h, r, obj, flt=flt, targets_fn=_cpu_targets,
                                  tie_counts_fn=_cpu_tie_counts)
        gt0, eq0 = sc.rank_ties_1vN(core, R, S, O_loc, h, r, obj, targets_fn=_cpu_targets, tie_counts_fn=_cpu_tie_counts)
        P = _scores(orc.query_vectors_ref(core, R, S, h, r), O)
        ref = tie_model.tie_counts(P.numpy(), obj.numpy(), known=lists)
        ref0 = tie_model.tie_counts(P.numpy(), obj.numpy())
        targets = torch.zeros_like(P)
        for d, l in enumerate(lists):
            targets[d, l] = 1.0
        stable = orc.filter_and_rank_stable(P, targets, obj).numpy()
        lo, hi = sc.shards.bounds(rank)
        owned = int(((obj >= lo) & (obj < hi)).sum())
        ok = (gt.dtype == torch.int32 and eq.dtype == torch.int32 and tuple(gt.shape) == (B,)
              and np.array_equal(gt.numpy(), ref[0]) and np.array_equal(eq.numpy(), ref[1])
              and np.array_equal(gt0.numpy(), ref0[0]) and np.array_equal(eq0.numpy(), ref0[1])
              and bool(((1 + ref[0] <= stable) & (stable <= 1 + ref[0] + ref[1])).all())
              and np.array_equal(stable, 1 + ref[0] + ref[2])
              and calls == [B, B])                    # stage 1 once per call, replicated
        q.put((rank, bool(ok), int(ref[1].max()), owned, bool(padded)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("far_targets", [False, True])
@pytest.mark.parametrize("n_ent", [64, 101])          # even shards; ragged last shard (padding rows are not entities)
def test_sharded_rank_ties_1vN_world2_gloo(n_ent, far_targets):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(rk, 2, port, n_ent, far_targets, q)) for rk in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = sorted(q.get(timeout=5) for _ in range(2))
    assert [r[1] for r in res] == [True, True], res
    assert res[0][2] >= 4, res                        # the repeated rows do tie: `equal` is not all zero
    assert res[1][4] == (n_ent == 101), res           # n_ent = 101: the last shard has a padding row
    if far_targets:
        assert res[1][3] == 0, res                    # rank 1 owned no target and still contributed its counts
