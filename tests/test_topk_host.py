"""Top-k link prediction without a GPU: the entity-sharded ``ShardedEntityScorer.topk`` under gloo with CPU stand-ins
for the select, ``DeviceFilter.slots_of`` on CPU tensors, and the argument checks of the ``rtk_select_topk_*`` entries
(return codes before anything touches a device)."""
import os
import socket
import types

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


def _oracle_local(core, R, S, O_loc, h, r, out, **kw):
    out.copy_(orc.score_ref(core, R, S, O_loc, h, r))
    return out


def _cpu_select(P, ids, k, lists=None, keep=None):
    """Best first by (value desc, id asc); ids < 0 absent; ids in lists[d] (except keep[d]) removed; (-inf, -1) padding."""
    B = P.shape[0]
    vals = torch.full((B, k), float("-inf"), dtype=torch.float32)
    out = torch.full((B, k), -1, dtype=torch.int64)
    for d in range(B):
        c = ids[d]
        m = c >= 0
        if lists is not None and lists[d] is not None:
            ex = torch.tensor([x for x in lists[d] if keep is None or x != int(keep[d])], dtype=torch.int64)
            m &= ~torch.isin(c, ex)
        v, c = P[d][m].double().numpy(), c[m].numpy()
        o = np.lexsort((c, -v))[:k]
        vals[d, :len(o)] = torch.from_numpy(v[o]).float()
        out[d, :len(o)] = torch.from_numpy(c[o])
    return vals, out


def _topk_worker(rank, world, port, n_ent, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from r_tucker_amd.sharded import ShardedEntityScorer
        n_rel, B, rank3, k = 5, 24, (3, 8, 8), 7
        core, R, S, O = [torch.from_numpy(x) for x in gen.make_params(n_ent, n_rel, rank3, 9)]
        O = (O * 8).round() / 8                       # coarse values -> exact ties between scores
        S = (S * 4).round() / 4
        h, r = [torch.from_numpy(x) for x in gen.make_queries(n_ent, n_rel, B, 9)]
        rng = np.random.default_rng(9)
        keep = torch.from_numpy(rng.integers(0, n_ent, B))
        lists = [sorted(set([int(keep[d])] + rng.integers(0, n_ent, rng.integers(0, 12)).tolist())) for d in range(B)]
        lists[3] = None                                        # a row without a filter list
        lists[5] = list(range(n_ent))                          # a row with every entity excluded -> all padding
        keep[5] = -1
        slots = torch.tensor([-1 if l is None else d for d, l in enumerate(lists)], dtype=torch.int64)
        calls = []

        def local(P, k_, col0, flt, slots_, keep_):
            calls.append((tuple(P.shape), col0))
            ids = col0 + torch.arange(P.shape[1], dtype=torch.int64).expand(P.shape[0], -1)
            return _cpu_select(P, ids, k_, [None if int(s) < 0 else lists[int(s)] for s in slots_], keep_)

        def merge(v, i, k_):
            assert tuple(v.shape) == (B, world * k_)
            return _cpu_select(v, i, k_)
        sc = ShardedEntityScorer(n_ent, local_score=_oracle_local)
        vals, ids = sc.topk(core, R, S, sc.local_block(O), h, r, k, flt=types.SimpleNamespace(), slots=slots,
                            keep_idx=keep, local_topk_fn=local, merge_fn=merge)
        P = orc.score_ref(core, R, S, O, h, r)
        rv, ri = _cpu_select(P, torch.arange(n_ent).expand(B, -1), k, lists, keep)
        lo, hi = sc.shards.bounds(rank)
        ok = (torch.equal(ids, ri) and torch.equal(vals, rv) and calls == [((B, hi - lo), rank * sc.shards.n_loc)]
              and bool((ids[5] == -1).all()))
        q.put((rank, bool(ok), int((ids != ri).sum())))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_ent", [101])                 # odd: the last shard has a padding row
def test_sharded_topk_world2_gloo(n_ent):
    """Shard-local select over the real columns + one all-gather of (B, k) lists + merge = the filtered stable sort
    of the full score matrix cut at k."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_topk_worker, args=(rk, 2, port, n_ent, q)) for rk in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = sorted(q.get(timeout=5) for _ in range(2))
    assert [r[1] for r in res] == [True, True], res


def test_slots_of_cpu():
    from r_tucker_amd.evaluation import DeviceFilter
    pairs = np.array([[4, 1], [0, 0], [2, 3], [0, 2]], dtype=np.int64)          # slot i = pairs[i]
    ptr = np.array([0, 2, 3, 5, 6], dtype=np.int64)
    obj = np.array([7, 8, 1, 2, 9, 3], dtype=np.int64)
    ds = types.SimpleNamespace(_pairs=pairs, _ptr=ptr, _obj=obj,
                               features=np.array([[0, 2, 3], [4, 1, 7]], dtype=np.int64))
    flt = DeviceFilter(ds, "cpu")
    h = torch.tensor([4, 0, 2, 0, 1, 4, -1, 2, 0, 9])
    r = torch.tensor([1, 0, 3, 2, 1, 0, 0, 4, -1, 1])
    got = flt.slots_of(h, r)
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    assert got.tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1, -1]
    assert torch.equal(flt.slots_of(flt.subj, flt.rel), flt.slot_of_item)
    assert flt.slots_of(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)).numel() == 0
    with pytest.raises(RuntimeError):
        flt.slots_of(torch.tensor([0, 1]), torch.tensor([0]))


@pytest.fixture(scope="module")
def lib():
    from r_tucker_amd import _lib
    return _lib.load()


def test_select_topk_argument_validation(lib):
    assert lib.rtk_version() >= 213
    assert lib.rtk_select_topk_workspace_bytes(512, 40943, 10) == 0
    for fn in (lib.rtk_select_topk_f32, lib.rtk_select_topk_bf16):
        # P, batch, n_cols, ld, col0, col_ids, ld_ids, pair_slot, pair_ptr, pair_obj, keep_idx, k, values, ids, ws, wsb, stream
        ok = [256, 4, 100, 128, 0, None, 0, None, None, None, None, 10, 256, 256, None, 0, None]

        def rc(**ch):
            a = list(ok)
            names = ["P", "batch", "n_cols", "ld", "col0", "col_ids", "ld_ids", "pair_slot", "pair_ptr", "pair_obj",
                     "keep_idx", "k", "values", "ids", "ws", "wsb", "stream"]
            for n_, v in ch.items():
                a[names.index(n_)] = v
            return fn(*a), lib.rtk_last_error_string()
        for k in (0, -1, 1025):
            code, msg = rc(k=k)
            assert code == -1 and b"k = " in msg
        for n_ in ("P", "values", "ids"):
            code, msg = rc(**{n_: None})
            assert code == -1 and b"null" in msg
        code, msg = rc(ld=99)
        assert code == -1 and b"bad sizes" in msg
        code, msg = rc(col0=-1)
        assert code == -1
        code, msg = rc(col_ids=256, ld_ids=50)
        assert code == -1 and b"ld_ids" in msg
        code, msg = rc(pair_slot=256)
        assert code == -1 and b"CSR" in msg
        code, _ = rc(n_cols=1 << 31, ld=1 << 31)
        assert code == -3
        assert rc(batch=0)[0] == 0                     # an empty batch enqueues nothing
