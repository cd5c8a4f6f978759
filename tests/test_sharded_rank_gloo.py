"""``ShardedEntityScorer.rank_1vN`` (ranking on entity shards without the score block) under the gloo backend,
world_size 2, on CPU.  The two block steps are injected as CPU functions that restate the rule of
``rtk_score_rank_targets_*`` / ``rtk_score_rank_counts_*`` on "packed" query vectors (here: the plain vectors), so the
host logic -- stage 1 once, ownership by global id, the padding rows of the last shard, the MAX and SUM all-reduces --
runs without a GPU.  The result must equal the oracle's stable filtered ranks on the full matrix."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gen
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


def _cpu_counts(v, B, O_loc, col0, n_ent, pt, obj, flt=None, slots=None, want_bce=False, sigmoid_mode=None):
    """#{j : p'_j > pt} + #{j < t : p'_j == pt} over the block's rows, j global; other known objects count as 0."""
    P = _scores(v, O_loc)
    n = O_loc.shape[0]
    counts = torch.zeros(B, dtype=torch.int32)
    bce = torch.zeros(B, dtype=torch.float64)
    for d in range(B):
        p = P[d].clone()
        t = int(obj[d])
        y = torch.zeros(n, dtype=torch.float64)
        if flt is not None and int(slots[d]) >= 0:
            s = int(slots[d])
            for g in flt.pair_obj[flt.pair_ptr[s]:flt.pair_ptr[s + 1]].tolist():
                if 0 <= g - col0 < n:
                    y[g - col0] = 1.0
                    if g != t:
                        p[g - col0] = 0.0
        elif 0 <= t - col0 < n:
            y[t - col0] = 1.0
        before = torch.arange(col0, col0 + n) < t
        mine = torch.arange(col0, col0 + n) == t
        counts[d] = int(((p > pt[d]) & ~mine).sum() + ((p == pt[d]) & before).sum())
        q = P[d].double()
        bce[d] = -(y * q.log().clamp(min=-100) + (1 - y) * (1 - q).log().clamp(min=-100)).sum()
    return (counts, bce) if want_bce else counts


def _rank_worker(rank, world, port, n_ent, far_targets, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from r_tucker_amd.sharded import ShardedEntityScorer
        n_rel, B, rank3 = 5, 24, (3, 8, 8)
        core, R, S, O = [torch.from_numpy(x) for x in gen.make_params(n_ent, n_rel, rank3, 9)]
        O = (O * 8).round() / 8                       # coarse values -> exact ties between scores
        S = (S * 4).round() / 4
        h, r = [torch.from_numpy(x) for x in gen.make_queries(n_ent, n_rel, B, 9)]
        rng = np.random.default_rng(9)
        # far_targets: every queried object lies in rank 0's shard, so rank 1 owns no target at all
        obj = torch.from_numpy(rng.integers(0, n_ent // 2 if far_targets else n_ent, B))
        # one filter list per query: the queried object plus up to 5 other known-true objects
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
        ranks, bce = sc.rank_1vN(core, R, S, O_loc, h, r, obj, flt=flt, want_bce=True, targets_fn=_cpu_targets,
                                 counts_fn=_cpu_counts)
        plain = sc.rank_1vN(core, R, S, O_loc, h, r, obj, targets_fn=_cpu_targets, counts_fn=_cpu_counts)
        P = _scores(orc.query_vectors_ref(core, R, S, h, r), O)
        targets = torch.zeros_like(P)
        for d, l in enumerate(lists):
            targets[d, l] = 1.0
        ref = orc.filter_and_rank_stable(P, targets, obj)
        only = torch.zeros_like(P)
        only[torch.arange(B), obj] = 1.0
        ref_plain = orc.filter_and_rank_stable(P, only, obj)
        P64 = P.double()
        ref_bce = -(targets.double() * P64.log().clamp(min=-100)
                    + (1 - targets.double()) * (1 - P64).log().clamp(min=-100)).sum(1)
        lo, hi = sc.shards.bounds(rank)
        owned = int(((obj >= lo) & (obj < hi)).sum())
        ok = (torch.equal(ranks.long(), ref.long()) and torch.equal(plain.long(), ref_plain.long())
              and ranks.dtype == torch.int32 and torch.allclose(bce, ref_bce, rtol=1e-9, atol=1e-9)
              and calls == [B, B])                    # stage 1 once per call, replicated
        q.put((rank, bool(ok), int((ranks.long() - ref.long()).abs().max()), owned))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("far_targets", [False, True])
@pytest.mark.parametrize("n_ent", [64, 101])          # even shards; ragged last shard (padding rows are not entities)
def test_sharded_rank_1vN_world2_gloo(n_ent, far_targets):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(rk, 2, port, n_ent, far_targets, q)) for rk in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = sorted(q.get(timeout=5) for _ in range(2))
    assert [r[1] for r in res] == [True, True], res
    if far_targets:
        assert res[1][3] == 0, res                    # rank 1 owned no target and still contributed its counts
