"""``ShardedEntityScorer.bce_loss_1vN`` (the training loss on entity shards without the score block) under the gloo
backend, world_size 2, on CPU.  The block steps are injected as float64 CPU functions that restate the rule of
``rtk_bce_stream_rows_part_f32`` / ``rtk_bce_stream_grad_o_part_f32`` (smoothing term ``eps / n_ent``, ownership of a
known object by its global id, local rows), so the host logic -- the real rows of a padded shard, a rank without rows,
one all-reduce of the loss rows in the forward and one of dv in the backward -- runs without a GPU.  Loss and
gradients must equal the oracle's on the full matrix at float64 round-off."""
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


def _block_x(v, O_loc, col0, n_ent, slot, ptr, obj, eps):
    """(z, y) of the block: float64 logits and the smoothed targets of its rows (CSR entries by global id)."""
    n = O_loc.shape[0]
    z = v @ O_loc.T
    y = torch.full_like(z, eps / n_ent)
    for d, s in enumerate(slot.tolist()):
        if s >= 0:
            for g in obj[ptr[s]:ptr[s + 1]].tolist():
                if 0 <= g - col0 < n:
                    y[d, g - col0] = eps / n_ent + (1.0 - eps)
    return z, y


def _cpu_rows(qp, B, O_loc, col0, n_ent, slot, ptr, obj, eps, sigmoid_mode, want_dv):
    z, y = _block_x(qp, O_loc.detach(), col0, n_ent, slot, ptr, obj, eps)
    ls = torch.nn.functional.logsigmoid
    rows = -(y * ls(z) + (1 - y) * ls(-z)).sum(1)
    return rows, ((torch.sigmoid(z) - y) @ O_loc.detach() if want_dv else None)


def _cpu_grad_o(qp, v, B, O_loc, col0, n_ent, slot, ptr, obj, max_pos, eps, sigmoid_mode, scale):
    z, y = _block_x(qp, O_loc.detach(), col0, n_ent, slot, ptr, obj, eps)
    return (torch.sigmoid(z) - y).T @ (v * scale)


def _cpu_stage1_bwd(core, R, S, h, r, dv, needs):
    leaves = [t.detach().clone().requires_grad_(True) for t in (core, R, S)]
    with torch.enable_grad():                    # called from inside an autograd backward
        orc.query_vectors_ref(*leaves, h, r).backward(dv)
    return tuple(t.grad if n else None for t, n in zip(leaves, needs))


def _case(n_ent):
    """Operands (float64), queries and one CSR list per query; S has its own row count."""
    n_rel, B, rank3 = 5, 12, (3, 8, 8)
    core, R, S, O = [torch.from_numpy(x).double() for x in gen.make_params(max(n_ent, 16), n_rel, rank3, 19)]
    O = O[:n_ent].contiguous()
    h, r = [torch.from_numpy(x) for x in gen.make_queries(S.shape[0], n_rel, B, 19)]
    rng = np.random.default_rng(19)
    lists = [sorted(set(rng.integers(0, n_ent, rng.integers(0, 6)).tolist())) for _ in range(B)]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64)
    obj = torch.tensor([x for l in lists for x in l], dtype=torch.int64)
    flt = SimpleNamespace(slot_of_item=torch.arange(B), pair_ptr=ptr, pair_obj=obj, max_list=max(1, max(map(len, lists))))
    y = torch.full((B, n_ent), EPS / n_ent, dtype=torch.float64)
    for d, l in enumerate(lists):
        y[d, l] += 1.0 - EPS
    return core, R, S, O, h, r, flt, y


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
            reduced.append(tuple(t.shape))
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
        loss = sc.bce_loss_1vN(*leaves, O_loc, h, r, flt, torch.arange(B), label_smoothing=EPS, rows_fn=_cpu_rows,
                               grad_o_fn=_cpu_grad_o, stage1_bwd_fn=_cpu_stage1_bwd)
        after_forward = list(reduced)
        (loss * 3.0).backward()
        lo, hi = sc.shards.bounds(rank)
        c = core.shape[2]
        counts_ok = (after_forward == [(B,)] and reduced == [(B,), (B, c)]          # one reduction each way
                     and stage1 == ([B] if hi > lo else []))                        # stage 1 once, replicated
        pad_ok = not bool(O_loc.grad[hi - lo:].any())                               # padding rows: zero gradient
        q.put((rank, float(loss), [t.grad.numpy() for t in leaves], O_loc.grad[: hi - lo].numpy(), bool(counts_ok),
               bool(pad_ok), hi - lo))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_ent", [101, 1])      # a ragged last shard (padding rows); rank 1 owns no row at all
def test_sharded_bce_loss_world2_gloo(n_ent):
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
    core, R, S, O, h, r, _, y = _case(n_ent)
    ref = orc.bce_loss_grads_ref(core, R, S, O, h, r, y)
    tol = 1e-10
    for rank, loss, grads, _, counts_ok, pad_ok, n_rows in res:
        assert counts_ok and pad_ok, res
        assert abs(loss - ref[0].item()) <= tol * abs(ref[0].item())
        for g, e in zip(grads, ref[1:4]):
            e = 3.0 * e.numpy()
            assert np.abs(g - e).max() <= tol * np.abs(e).max()
    if n_ent == 1:
        assert res[1][6] == 0                    # rank 1 owned no row and still took part in both reductions
    for a, b in zip(res[0][2], res[1][2]):       # complete and EQUAL on the two ranks
        assert np.array_equal(a, b)
    gO = np.concatenate([res[0][3], res[1][3]], axis=0)
    e = 3.0 * ref[4].numpy()
    assert gO.shape == e.shape and np.abs(gO - e).max() <= tol * np.abs(e).max()
