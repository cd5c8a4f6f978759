"""``ShardedEntityScorer.ce_loss_1vN`` (the softmax cross-entropy loss on entity shards without the logit block) under
the gloo backend, world_size 2, on CPU.  The block steps are injected as float64 CPU functions that restate the rule of
``rtk_ce_stream_rows_part_f32`` / ``rtk_ce_stream_grad_part_f32`` (smoothing term ``eps / n_ent``, ``n_d`` the whole
list's length, ownership of a known object by its global id, local rows, the backward from the GLOBAL lse), so the host
logic -- the real rows of a padded shard, a rank without rows, the MAX and the SUM of the forward and the SUM of dv in
the backward -- runs without a GPU.  Loss and gradients must equal ``F.cross_entropy`` on the full matrix at float64
round-off."""
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gen
from oracle import score_oracle as orc

EPS = 0.1


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _targets(B, n, col0, n_ent, slot, ptr, obj, eps):
    """(y of the block's n columns, the rows' mass w): n_d is the whole list's length."""
    y = torch.full((B, n), eps / n_ent, dtype=torch.float64)
    w = torch.full((B,), eps, dtype=torch.float64)
    for d, s in enumerate(slot.tolist()):
        if s >= 0 and ptr[s + 1] > ptr[s]:
            l = obj[ptr[s]:ptr[s + 1]].tolist()
            w[d] += 1.0 - eps
            for g in l:
                if 0 <= g - col0 < n:
                    y[d, g - col0] += (1.0 - eps) / len(l)
    return y, w


def _cpu_partials(qp, B, O_loc, col0, n_ent, slot, ptr, obj, eps):
    z = qp @ O_loc.detach().T
    y, _ = _targets(B, O_loc.shape[0], col0, n_ent, slot, ptr, obj, eps)
    m = z.max(dim=1).values
    return m, torch.exp(z - m[:, None]).sum(dim=1), -(y * z).sum(dim=1)


def _cpu_grad(qp, v, B, O_loc, col0, n_ent, slot, ptr, obj, max_pos, eps, lse, scale, want_dv, want_gO):
    O_ = O_loc.detach()
    z = qp @ O_.T
    y, w = _targets(B, O_.shape[0], col0, n_ent, slot, ptr, obj, eps)
    x = w[:, None] * torch.exp(z - lse[:, None]) - y
    return (x @ O_ if want_dv else None), (x.T @ (v * scale) if want_gO else None)


def _cpu_stage1_bwd(core, R, S, h, r, dv, needs):
    leaves = [t.detach().clone().requires_grad_(True) for t in (core, R, S)]
    with torch.enable_grad():                    # called from inside an autograd backward
        orc.query_vectors_ref(*leaves, h, r).backward(dv)
    return tuple(t.grad if n else None for t, n in zip(leaves, needs))


def _case(n_ent):
    """Operands (float64), queries and one CSR list per query (some empty); S has its own row count."""
    n_rel, B, rank3 = 5, 12, (3, 8, 8)
    core, R, S, O = [torch.from_numpy(x).double() for x in gen.make_params(max(n_ent, 16), n_rel, rank3, 23)]
    O = O[:n_ent].contiguous()
    h, r = [torch.from_numpy(x) for x in gen.make_queries(S.shape[0], n_rel, B, 23)]
    rng = np.random.default_rng(23)
    lists = [sorted(set(rng.integers(0, n_ent, rng.integers(0, 6)).tolist())) for _ in range(B)]
    if n_ent > 60:
        lists[0] = [3, 50, n_ent - 1]            # entries on both ranks
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64)
    obj = torch.tensor([x for l in lists for x in l], dtype=torch.int64)
    flt = SimpleNamespace(slot_of_item=torch.arange(B), pair_ptr=ptr, pair_obj=obj, max_list=max(1, max(map(len, lists))))
    y = torch.full((B, n_ent), EPS / n_ent, dtype=torch.float64)
    for d, l in enumerate(lists):
        if l:
            y[d, l] += (1.0 - EPS) / len(l)
    return core, R, S, O, h, r, flt, y


def _reference(n_ent):
    core, R, S, O, h, r, _, y = _case(n_ent)
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
    z = orc.query_vectors_ref(*leaves[:3], h, r) @ leaves[3].T
    loss = torch.nn.functional.cross_entropy(z, y)
    (3.0 * loss).backward()
    return loss.item(), [t.grad.numpy() for t in leaves]


def _loss_worker(rank, world, port, n_ent, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from r_tucker_amd.sharded import ShardedEntityScorer
        core, R, S, O, h, r, flt, _ = _case(n_ent)
        B = h.numel()
        reduced = []
        real_all_reduce = dist.all_reduce

        def counting_all_reduce(t, *a, **kw):
            reduced.append((tuple(t.shape), kw.get("op")))
            return real_all_reduce(t, *a, **kw)
        dist.all_reduce = counting_all_reduce

        stage1 = []

        def qv(core_, R_, S_, hh, rr, **kw):
            stage1.append(int(hh.numel()))
            return orc.query_vectors_ref(core_.detach(), R_.detach(), S_.detach(), hh, rr)

        sc = ShardedEntityScorer(n_ent, query_vectors_fn=qv)
        sc.pack_fn = lambda v, dtype: v
        leaves = [t.clone().requires_grad_(True) for t in (core, R, S)]
        O_loc = sc.local_block(O).requires_grad_(True)
        loss = sc.ce_loss_1vN(*leaves, O_loc, h, r, flt, torch.arange(B), label_smoothing=EPS, partials_fn=_cpu_partials,
                              grad_fn=_cpu_grad, stage1_bwd_fn=_cpu_stage1_bwd)
        after_forward = list(reduced)
        (loss * 3.0).backward()
        lo, hi = sc.shards.bounds(rank)
        c = core.shape[2]
        MAX, SUM = dist.ReduceOp.MAX, dist.ReduceOp.SUM
        fwd = [((B,), MAX), ((2, B), SUM)]
        counts_ok = (after_forward == fwd and reduced == fwd + [((B, c), SUM)]        # exactly the three exchanges
                     and stage1 == ([B] if hi > lo else []))                        # stage 1 once, replicated
        pad_ok = not bool(O_loc.grad[hi - lo:].any())                               # padding rows: zero gradient
        q.put((rank, float(loss), [t.grad.numpy() for t in leaves], O_loc.grad[: hi - lo].numpy(), bool(counts_ok),
               bool(pad_ok), hi - lo))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_ent", [101, 1])      # a ragged last shard (padding rows); rank 1 owns no row at all
def test_sharded_ce_loss_world2_gloo(n_ent):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_loss_worker, args=(rk, 2, port, n_ent, q)) for rk in range(2)]
    res = []
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=120) for _ in range(2)), key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(120)
    assert all(p.exitcode == 0 for p in procs)
    ref_loss, ref_grads = _reference(n_ent)
    tol = 1e-10
    for rank, loss, grads, _, counts_ok, pad_ok, n_rows in res:
        assert counts_ok and pad_ok, res
        assert abs(loss - ref_loss) <= tol * abs(ref_loss)
        for g, e in zip(grads, ref_grads[:3]):
            assert np.abs(g - e).max() <= tol * np.abs(e).max()
    if n_ent == 1:
        assert res[1][6] == 0                    # rank 1 owned no row and still took part in all three exchanges
    for a, b in zip(res[0][2], res[1][2]):       # complete and EQUAL on the two ranks
        assert np.array_equal(a, b)
    gO = np.concatenate([res[0][3], res[1][3]], axis=0)
    e = ref_grads[3]
    assert gO.shape == e.shape and np.abs(gO - e).max() <= tol * np.abs(e).max()
