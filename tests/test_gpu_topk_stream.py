"""GPU tests of filtered top-k link prediction without the score matrix (ops.topk_1vN(matrix_free=True),
ops.topk_block_1vN, rtk_score_topk_*, csrc/rtk_score_topk.hip).

The reference in every case is evaluation.filtered_topk (rtk_select_topk_f32) on the matrix the stored score kernel
writes from the same packed query planes: for fp32 operands the ws kernel's (RTK_SCORE_KERNEL_WS), for bf16 operands
rtk_score_packed_bf16's.  The checks are exact: ids equal, values equal as bit patterns."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


class Flt:
    """Stand-in for DeviceFilter: a CSR of known objects and the slot of each query (-1: none)."""

    def __init__(self, lists, slots):
        lists = list(lists) or [[]]
        self.pair_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64).cuda()
        # (one unused entry behind the last list: an all-empty CSR still has a non-null array)
        self.pair_obj = torch.tensor(np.concatenate([np.asarray(x, dtype=np.int64) for x in lists] + [np.zeros(1, np.int64)]),
                                     dtype=torch.int64).cuda()
        self.slots = torch.as_tensor(slots, dtype=torch.int64).cuda()

    def slots_of(self, h, r):
        return self.slots


def _flags(rt, mode):
    L = rt._lib
    return L.RTK_SCORE_SIGMOID | (L.RTK_SCORE_SIGMOID_FAST if mode == "fast" else 0)


def _stored_scores(rt, qp, B, O, mode):
    """(B, N) fp32 probabilities from the stored score kernel (tests/test_gpu_rank.py obtains its reference so)."""
    lib = rt._lib.load()
    O = O.contiguous()
    N, c = O.shape
    P = torch.empty((B, N), dtype=torch.float32, device=O.device)
    sp = torch.cuda.current_stream().cuda_stream
    if O.dtype == torch.bfloat16:
        rt._lib.check(lib.rtk_score_packed_bf16(qp.data_ptr(), B, c, O.data_ptr(), N, P.data_ptr(), N, _flags(rt, mode), sp),
                      "bf16")
    else:
        rt._lib.check(lib.rtk_score_packed_f32(qp.data_ptr(), B, c, O.data_ptr(), N, P.data_ptr(), N,
                                               _flags(rt, mode) | rt._lib.RTK_SCORE_KERNEL_WS, sp), "ws")
    return P


def _problem(N, c, B, seed, dtype=torch.float32, gain=1.0, n_rel=5, a=6):
    g = torch.Generator().manual_seed(seed)
    core = (torch.randn(a, c, c, generator=g) / c).cuda()
    R = torch.randn(n_rel, a, generator=g).cuda()
    S = torch.randn(N, c, generator=g).cuda()
    O = (torch.randn(N, c, generator=g) * gain).cuda()
    h = torch.randint(0, N, (B,), generator=g).cuda()
    r = torch.randint(0, n_rel, (B,), generator=g).cuda()
    if dtype != torch.float32:
        core, R, S, O = core.to(dtype), R.to(dtype), S.to(dtype), O.to(dtype)
    return core, R, S, O, h, r


def _filter(N, B, seed, per=12):
    """Per query: no slot, an empty list, lists of random objects (some outside [0, N), some listed twice); keep_idx
    keeps a listed object for some queries."""
    rng = np.random.default_rng(seed + 1)
    lists, slots, keep = [], [], []
    for d in range(B):
        if d % 5 == 0:
            slots.append(-1)
            keep.append(-1)
            continue
        m = 0 if d % 5 == 4 else int(rng.integers(1, per + 1))
        objs = rng.integers(0, N, size=m).tolist()
        if d % 5 == 2:
            objs.append(N + 5)
        keep.append(objs[0] if objs and d % 5 == 3 else -1)
        slots.append(len(lists))
        lists.append(objs)
    return Flt(lists, slots), torch.tensor(keep, dtype=torch.int64).cuda()


def _same(got, ref):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[0].shape == ref[0].shape
    assert torch.equal(got[1], ref[1])
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))


def _check(rt, core, R, S, O, h, r, k, flt, keep, mode):
    """matrix-free top k of the whole range against the select on the stored kernel's matrix"""
    B = h.numel()
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, B, O, mode)
    slots = flt.slots_of(h, r) if flt is not None else None
    ref = rt.filtered_topk(P, k, flt, slots=slots, keep_idx=keep)
    got = rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, sigmoid_mode=mode, matrix_free=True)
    _same(got, ref)
    return P, got


SHAPES_F32 = [
    # (N, c, B, k): a partial last tile, fewer tiles than k (every tile selected), every k-step count at its edge
    (1, 4, 1, 1), (1, 36, 33, 10), (127, 4, 70, 128), (128, 36, 1, 10), (129, 200, 33, 1), (129, 208, 70, 10),
    (1000, 4, 33, 10), (1000, 36, 70, 1), (1000, 200, 70, 128), (1000, 208, 1, 10), (1000, 200, 33, 10),
    (2000, 36, 33, 10),           # more tiles than k = 10: tiles are really left out
    (70000, 16, 33, 10),          # more tiles than workgroup slots: a slot walks several tiles
    (384, 36, 200, 10),           # fewer tiles than slots: the query tiles are cut into ranges
]


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B,k", SHAPES_F32)
def test_f32_equals_select_on_ws_scores(rt, N, c, B, k, mode):
    core, R, S, O, h, r = _problem(N, c, B, N + c + B, gain=3.0)
    flt, keep = _filter(N, B, N + k)
    _check(rt, core, R, S, O, h, r, k, None, None, mode)
    _check(rt, core, R, S, O, h, r, k, flt, keep, mode)


SHAPES_BF16 = [(1, 8, 1, 1), (129, 8, 33, 10), (1000, 200, 70, 10), (1000, 512, 33, 128), (1000, 20, 33, 10),  # c % 8 != 0
               (127, 200, 70, 1), (2000, 512, 33, 10)]


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B,k", SHAPES_BF16)
def test_bf16_equals_select_on_bf16_kernel_scores(rt, N, c, B, k, mode):
    core, R, S, O, h, r = _problem(N, c, B, N + c + B, dtype=torch.bfloat16, gain=3.0)
    flt, keep = _filter(N, B, N + k)
    _check(rt, core, R, S, O, h, r, k, None, None, mode)
    _check(rt, core, R, S, O, h, r, k, flt, keep, mode)


def test_ties_take_the_lowest_eligible_ids(rt):
    """O = 0: every probability is 0.5, so the ids are the lowest eligible ones, in order."""
    N, c, B, k = 1000, 36, 33, 10
    core, R, S, O, h, r = _problem(N, c, B, 1)
    O.zero_()
    lists = [[0, 1, 5, 128, 129] if d % 2 else [] for d in range(B)]
    flt = Flt(lists, list(range(B)))
    P, (vals, ids) = _check(rt, core, R, S, O, h, r, k, flt, None, "exact")
    assert bool((P == 0.5).all())
    assert ids[0].tolist() == list(range(10)) and ids[1].tolist() == [2, 3, 4, 6, 7, 8, 9, 10, 11, 12]
    assert bool((vals == 0.5).all())
    # k tiles of 128 ties each, and the cut-off tie split inside a tile that is not the first
    lists = [list(range(0, 300)) for _ in range(B)]
    _, (_, ids) = _check(rt, core, R, S, O, h, r, k, Flt(lists, list(range(B))), None, "fast")
    assert ids[0].tolist() == list(range(300, 310))


def test_duplicated_rows_on_both_sides_of_a_tile_boundary(rt):
    N, c, B, k = 1000, 36, 33, 10
    core, R, S, O, h, r = _problem(N, c, B, 2, gain=3.0)
    O[120:136] = O[300]                         # 16 equal rows across the boundary at 128, equal to row 300's
    O[255] = O[256] = O[511] = O[512] = O[7]
    for mode in ("fast", "exact"):
        _check(rt, core, R, S, O, h, r, k, None, None, mode)
        _check(rt, core, R, S, O, h, r, 128, None, None, mode)


def test_padding_when_the_filter_leaves_fewer_than_k(rt):
    N, c, B, k = 300, 36, 33, 10
    core, R, S, O, h, r = _problem(N, c, B, 3, gain=3.0)
    lists = [[j for j in range(N) if j not in (7, 130, 299)][: N - 3 + (d % 2)] for d in range(B)]
    lists[2] = list(range(N))                   # nothing left
    flt = Flt(lists, list(range(B)))
    _, (vals, ids) = _check(rt, core, R, S, O, h, r, k, flt, None, "fast")
    assert sorted(ids[0, :3].tolist()) == [7, 130, 299] and ids[0, 3:].tolist() == [-1] * 7
    assert bool(torch.isneginf(vals[0, 3:]).all()) and ids[2].tolist() == [-1] * k and bool(torch.isneginf(vals[2]).all())


def test_filter_removes_the_best_entity_of_the_best_tiles(rt):
    """What the patch step exists for: with the unfiltered maxima the wrong tiles would be chosen."""
    N, c, B, k = 4000, 36, 33, 3
    core, R, S, O, h, r = _problem(N, c, B, 4, gain=3.0)
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, B, O, "fast")
    order = torch.argsort(P, dim=1, descending=True, stable=True).cpu().numpy()
    # the 6 best entities of every query (several tiles' maxima; some share a tile) are filtered
    lists = [order[d, :6].tolist() for d in range(B)]
    flt = Flt(lists, list(range(B)))
    _, (vals, ids) = _check(rt, core, R, S, O, h, r, k, flt, None, "fast")
    for d in range(B):
        assert ids[d].tolist() == order[d, 6:6 + k].tolist()
    # the tiles of the filtered best entities are not all among the tiles of the answer
    assert any(set(order[d, :6] // 128) - set(order[d, 6:6 + k] // 128) for d in range(B))


def test_several_filtered_entities_in_one_tile_and_keep_idx(rt):
    N, c, B, k = 1000, 36, 33, 10
    core, R, S, O, h, r = _problem(N, c, B, 5, gain=3.0)
    lists = [list(range(128 * (d % 7), 128 * (d % 7) + 100)) + [128 * (d % 7) + 3] for d in range(B)]   # one listed twice
    flt = Flt(lists, list(range(B)))
    keep = torch.tensor([128 * (d % 7) + 50 if d % 2 else -1 for d in range(B)]).cuda()
    for mode in ("fast", "exact"):
        _, (_, ids) = _check(rt, core, R, S, O, h, r, 128, flt, keep, mode)
        for d in range(B):
            row = set(ids[d].tolist())
            assert not row & (set(lists[d]) - {int(keep[d])})
    # a long list: more than one 64-entry chunk names the same tiles
    lists = [np.random.default_rng(d).permutation(600).tolist() for d in range(B)]
    _check(rt, core, R, S, O, h, r, k, Flt(lists, list(range(B))), keep, "fast")


def test_nan_row_ranks_first(rt):
    N, c, B, k = 1000, 36, 33, 10
    core, R, S, O, h, r = _problem(N, c, B, 6, gain=3.0)
    O[200, 3] = float("nan")
    O[900, 0] = float("nan")
    _, (vals, ids) = _check(rt, core, R, S, O, h, r, k, None, None, "exact")
    assert ids[:, :2].tolist() == [[200, 900]] * B and bool(torch.isnan(vals[:, :2]).all())
    flt = Flt([[200]], [0] * B)
    _, (_, ids) = _check(rt, core, R, S, O, h, r, k, flt, None, "fast")
    assert ids[:, 0].tolist() == [900] * B


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cuts", [(0, 1, 1000), (0, 777, 1000), (0, 130, 131, 1000), (0, 500, 999, 1000)])
def test_blocks_merge_to_the_whole_range(rt, cuts, dtype):
    """topk_block_1vN over a partition, merged as topk_1vN's block loop merges, equals the whole range exactly."""
    N, c, B, k = 1000, 36, 70, 10
    core, R, S, O, h, r = _problem(N, c, B, 7, dtype=dtype, gain=3.0)
    flt, keep = _filter(N, B, 7)
    slots = flt.slots_of(h, r)
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    whole = rt.topk_block_1vN(qp, B, O, 0, N, k, flt=flt, slots=slots, keep_idx=keep)
    _same(whole, rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True))
    vals = ids = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        bv, bi = rt.topk_block_1vN(qp, B, O[lo:hi], lo, N, k, flt=flt, slots=slots, keep_idx=keep)
        _same((bv, bi), rt.filtered_topk(_stored_scores(rt, qp, B, O[lo:hi], rt.ops.DEFAULT_SIGMOID), k, flt, slots=slots,
                                         keep_idx=keep, col0=lo))
        vals, ids = (bv, bi) if vals is None else rt.filtered_topk(torch.cat([vals, bv], 1), k, ids=torch.cat([ids, bi], 1))
    _same((vals, ids), whole)


def test_query_chunks_are_exact(rt, monkeypatch):
    N, c, B, k = 1000, 36, 200, 10
    core, R, S, O, h, r = _problem(N, c, B, 8, gain=3.0)
    flt, keep = _filter(N, B, 8)
    ref = rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True)
    need = rt._lib.load().rtk_score_topk_workspace_bytes(0, 64, N, c, k)
    monkeypatch.setattr(rt.ops, "TOPK_STREAM_WS_BYTES", need + 2000)
    assert rt.ops._topk_stream_chunk(0, B, N, c, k) == 64
    _same(rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True), ref)


def test_deterministic(rt):
    N, c, B, k = 2000, 200, 70, 10
    core, R, S, O, h, r = _problem(N, c, B, 9, gain=3.0)
    flt, keep = _filter(N, B, 9)
    a = rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True)
    b = rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True)
    _same(a, b)


def test_graph_capture(rt):
    N, c, B, k = 2000, 36, 70, 10
    core, R, S, O, h, r = _problem(N, c, B, 10, gain=3.0)
    flt, keep = _filter(N, B, 10)
    slots = flt.slots_of(h, r)
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    eager = rt.topk_block_1vN(qp, B, O, 0, N, k, flt=flt, slots=slots, keep_idx=keep, sigmoid_mode="fast")
    lib = rt._lib.load()
    ws = torch.zeros(lib.rtk_score_topk_workspace_bytes(0, B, N, c, k), dtype=torch.uint8, device="cuda")
    vals = torch.zeros((B, k), dtype=torch.float32, device="cuda")
    ids = torch.zeros((B, k), dtype=torch.int64, device="cuda")

    def call():
        rt._lib.check(lib.rtk_score_topk_f32(qp.data_ptr(), B, c, O.data_ptr(), N, 0, N, slots.data_ptr(), flt.pair_ptr.data_ptr(),
                                             flt.pair_obj.data_ptr(), keep.data_ptr(), k, _flags(rt, "fast"), vals.data_ptr(),
                                             ids.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream), "rtk_score_topk_f32")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                 # first use outside the capture (function attributes)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    vals.zero_()
    ids.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _same((vals, ids), eager)


@pytest.mark.parametrize("sym", [False, True])
def test_model_predict_forwards_matrix_free(rt, sym):
    n_ent, n_rel, rank, B, k = 1500, 5, (6, 36, 36), 70, 10
    core, R, S, O, h, r = _problem(n_ent, rank[1], B, 11, gain=3.0, n_rel=n_rel, a=rank[0])
    if sym:
        model = rt.SymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": core.cpu(), "R.weight": R.cpu(), "E.weight": O.cpu()})
    else:
        model = rt.AsymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": core.cpu(), "R.weight": R.cpu(), "S.weight": S.cpu(), "O.weight": O.cpu()})
    model.cuda().eval()
    flt, keep = _filter(n_ent, B, 11)
    E = model.E.weight if sym else model.O.weight
    Sw = model.E.weight if sym else model.S.weight
    got = model.predict(h, r, k=k, flt=flt, keep_idx=keep, matrix_free=True)
    _same(got, rt.topk_1vN(model.core, model.R.weight, Sw, E, h, r, k, flt=flt, keep_idx=keep, matrix_free=True))
    _check(rt, model.core.data, model.R.weight.data, Sw.data, E.data, h, r, k, flt, keep, rt.ops.DEFAULT_SIGMOID)


def test_sharded_scorer_without_a_process_group(rt):
    N, c, B, k = 1500, 36, 70, 10
    core, R, S, O, h, r = _problem(N, c, B, 12, gain=3.0)
    flt, keep = _filter(N, B, 12)
    sc = rt.ShardedEntityScorer(N)
    got = sc.topk(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True)
    _same(got, rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=True))


def test_limits_raise_with_their_numbers(rt):
    core, R, S, O, h, r = _problem(300, 36, 4, 13)
    with pytest.raises(ValueError, match="128"):
        rt.topk_1vN(core, R, S, O, h, r, 129, matrix_free=True)
    with pytest.raises(ValueError, match="128"):
        rt.topk_1vN(core, R, S, O, h, r, 0, matrix_free=True)
    with pytest.raises(ValueError, match="entity_block"):
        rt.topk_1vN(core, R, S, O, h, r, 10, matrix_free=True, entity_block=100)
    with pytest.raises(ValueError, match="float32"):
        rt.topk_1vN(core, R, S, O, h, r, 10, matrix_free=True, score_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="probabilities"):
        rt.topk_1vN(core, R, S, O, h, r, 10, matrix_free=True, sigmoid=False)
    with pytest.raises(ValueError, match="fast.*exact"):
        rt.topk_1vN(core, R, S, O, h, r, 10, matrix_free=True, sigmoid_mode="approximate")
    big = _problem(50, 212, 4, 13)
    with pytest.raises(RuntimeError, match="208"):
        rt.topk_1vN(*big, 10, matrix_free=True)
    odd = _problem(50, 6, 4, 13)
    with pytest.raises(RuntimeError, match="c % 4 == 0"):
        rt.topk_1vN(*odd, 10, matrix_free=True)
    # the C ABI itself refuses them, with the numbers, before anything is enqueued
    lib = rt._lib.load()
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out_v, out_i = torch.zeros(4, 129, device="cuda"), torch.zeros(4, 129, dtype=torch.int64, device="cuda")
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)

    def abi(fn, c_, O_, k_, flags):
        return fn(qp.data_ptr(), 4, c_, O_.data_ptr(), O_.shape[0], 0, O_.shape[0], None, None, None, None, k_, flags,
                  out_v.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert abi(lib.rtk_score_topk_f32, 36, O, 129, 5) == -1 and b"128" in lib.rtk_last_error_string()
    assert abi(lib.rtk_score_topk_f32, 36, O, 10, 0) == -3 and b"RTK_SCORE_SIGMOID" in lib.rtk_last_error_string()
    assert abi(lib.rtk_score_topk_f32, 212, big[3], 10, 5) == -3 and b"208" in lib.rtk_last_error_string()
    assert abi(lib.rtk_score_topk_bf16, 528, torch.zeros(50, 528, dtype=torch.bfloat16, device="cuda"), 10, 5) == -3
    assert b"512" in lib.rtk_last_error_string()
    bf = _problem(50, 520, 4, 13, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="512"):
        rt.topk_block_1vN(torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"), 4, bf[3], 0, 50, 10)


def test_defaults_unchanged(rt):
    N, c, B, k = 1500, 36, 70, 10
    core, R, S, O, h, r = _problem(N, c, B, 14, gain=3.0)
    flt, keep = _filter(N, B, 14)
    for kw in ({}, {"entity_block": 400}, {"sigmoid": False}):
        a = rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, **kw)
        a = (a[0].clone(), a[1].clone())
        _same(a, rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, matrix_free=False, **kw))
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = rt.score_1vN(core, R, S, O, h, r)
    _same(rt.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep), rt.filtered_topk(P, k, flt, slots=flt.slots, keep_idx=keep))


def test_wn18rr_shape(rt):
    """The one case at full size: N 40 943, B 512, rank (10, 200, 200), k 10, the filter of the train split."""
    import gen
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    ds = KG_dataset(data, data.train_data)
    n_ent, n_rel, rank = len(data.entities), len(data.relations), (10, 200, 200)
    core, R, S, O = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, rank, 322, logit_std=3.0)]
    flt = rt.DeviceFilter(ds, "cuda")
    f = flt.features[torch.arange(0, 512 * 7, 7, device="cuda")]          # (subject, relation) pairs of the train split
    h, r = f[:, 0].contiguous(), f[:, 1].contiguous()
    slots = flt.slots_of(h, r)
    assert n_ent == 40943 and h.numel() == 512 and bool((slots >= 0).all())
    t = flt.pair_obj[flt.pair_ptr[slots]]                                  # each pair's first known object
    for keep in (None, t):
        _check(rt, core, R, S, O, h, r, 10, flt, keep, "fast")
