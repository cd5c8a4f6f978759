"""Filtered top-k selection on the MI355X (rtk_select_topk_*, evaluation.filtered_topk, ops.topk_1vN, model.predict):
exact comparison, no tolerances, against a numpy reference -- np.lexsort on (id, canonicalised value) after removing
the excluded columns."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- reference --------------------------------------------------------------------------------------------------
def _keys(v):
    """Order-preserving integer keys of float32 values: -0 == +0, every NaN above +inf, all NaNs equal."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC00000, u)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _canon(v):
    v = np.asarray(v, dtype=np.float32).copy()
    v[np.isnan(v)] = np.nan
    v[v == 0] = 0.0
    return v


def ref_topk(P, k, col0=0, ids=None, lists=None, keep=None):
    """P: (B, n) float32 numpy; ids: (B, n) int64 (merge mode) or None; lists: per-row excluded ids (or None)."""
    B, n = P.shape
    vals = np.full((B, k), -np.inf, dtype=np.float32)
    out = np.full((B, k), -1, dtype=np.int64)
    for d in range(B):
        cid = ids[d].copy() if ids is not None else col0 + np.arange(n, dtype=np.int64)
        m = cid >= 0
        if lists is not None and lists[d] is not None:
            ex = np.asarray(sorted(set(lists[d]) - ({int(keep[d])} if keep is not None else set())), dtype=np.int64)
            m &= ~np.isin(cid, ex)
        v, c = P[d][m], cid[m]
        o = np.lexsort((c, -_keys(v)))[:k]
        vals[d, :len(o)] = _canon(v[o])
        out[d, :len(o)] = c[o]
    return vals, out


def _same(got, ref):
    gv, gi = [t.cpu().numpy() for t in got]
    rv, ri = ref
    assert np.array_equal(gi, ri), np.argwhere(gi != ri)[:5]
    assert np.array_equal(gv, rv, equal_nan=True)
    assert np.array_equal(np.signbit(gv[gv == 0]), np.zeros(int((gv == 0).sum()), bool))   # +0.0 written


def _values(kind, B, n, rng):
    if kind == "cont":
        return rng.standard_normal((B, n)).astype(np.float32)
    if kind == "quant":
        return (rng.integers(0, 4, (B, n)) / 4).astype(np.float32)
    if kind == "equal":
        return np.full((B, n), 0.5, dtype=np.float32)
    # specials sprinkled into a few levels: +-0, +-inf, NaNs of both signs and several payloads
    P = (rng.integers(-2, 3, (B, n)) / 2).astype(np.float32)
    sp = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA00000],
                  dtype=np.uint32).view(np.float32)
    mask = rng.random((B, n)) < 0.2
    P[mask] = sp[rng.integers(0, len(sp), int(mask.sum()))]
    return P


def _flt(lists, dev):
    """A filter with one CSR slot per row (None -> slot -1)."""
    ptr, obj, slots = [0], [], []
    for l in lists:
        if l is None:
            slots.append(-1)
            continue
        slots.append(len(ptr) - 1)
        obj += list(l)
        ptr.append(len(obj))
    f = types.SimpleNamespace(pair_ptr=torch.tensor(ptr, dtype=torch.int64, device=dev),
                              pair_obj=torch.tensor(obj, dtype=torch.int64, device=dev))
    return f, torch.tensor(slots, dtype=torch.int64, device=dev)


def _device_matrix(P, dtype, ld_extra):
    B, n = P.shape
    buf = torch.full((B, n + ld_extra), 7.0, dtype=dtype, device="cuda")     # padding columns are never candidates
    buf[:, :n] = torch.from_numpy(P).to(dtype)
    return buf[:, :n]


CASES = [  # (B, n, ld_extra, col0, k, values)
    (1, 1, 0, 0, 1, "cont"), (1, 1, 3, 5, 10, "cont"), (7, 63, 1, 0, 10, "quant"), (7, 64, 0, 100, 100, "special"),
    (7, 63, 5, 0, 1024, "cont"), (512, 40943, 17, 0, 10, "cont"), (512, 40943, 17, 0, 1024, "quant"),
    (7, 40943, 0, 3, 100, "equal"), (7, 40943, 1, 0, 1024, "special"), (7, 125000, 8, 1000, 10, "cont"),
    (7, 125000, 0, 0, 1024, "quant"), (1, 125000, 0, 0, 100, "equal"), (7, 125000, 3, 7, 100, "special"),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_select_engineered(case, dtype):
    from r_tucker_amd.evaluation import filtered_topk
    B, n, ld_extra, col0, k, kind = case
    rng = np.random.default_rng(B * 131 + n + k)
    P = _values(kind, B, n, rng)
    Pd = _device_matrix(P, dtype, ld_extra)
    P = Pd.float().cpu().numpy()              # what the kernel sees (bf16-rounded)
    before = Pd.clone()
    _same(filtered_topk(Pd, k, col0=col0), ref_topk(P, k, col0))
    # exclusion: a list longer than k and than one bitmap window's worth of ids, out-of-block ids, keep_idx inside a
    # list, a row with every column excluded, rows without a list
    lists, keep = [], np.full(B, -1, dtype=np.int64)
    for d in range(B):
        if d % 4 == 3:
            lists.append(None)
            continue
        if d % 4 == 2:
            lists.append(list(range(col0, col0 + n)))
            continue
        m = min(n, max(3 * k, 5000) if d % 4 == 0 else 7)
        l = (col0 + rng.choice(n, m, replace=False)).tolist() + [col0 - 1, col0 + n, col0 + n + 5]
        lists.append(l)
        keep[d] = l[0] if d % 2 == 0 else col0 + int(rng.integers(0, n))
    flt, slots = _flt(lists, "cuda")
    kp = torch.from_numpy(keep).cuda()
    _same(filtered_topk(Pd, k, flt, slots=slots, keep_idx=kp, col0=col0), ref_topk(P, k, col0, lists=lists, keep=keep))
    assert torch.equal(Pd.view(torch.int16) if dtype == torch.bfloat16 else Pd.view(torch.int32),
                       before.view(torch.int16) if dtype == torch.bfloat16 else before.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["cont", "quant", "special"])
def test_merge_mode(kind, dtype):
    """Two blocks' top-k lists concatenated (ids in ascending ranges, some absent) merge to the top k of the union."""
    from r_tucker_amd.evaluation import filtered_topk
    B, n, k = 33, 3000, 100
    rng = np.random.default_rng(5)
    Pd = _device_matrix(_values(kind, B, n, rng), dtype, 0)
    P = Pd.float().cpu().numpy()
    half = n // 2 + 1
    a = filtered_topk(Pd[:, :half], k, col0=0)
    b = filtered_topk(Pd[:, half:], k, col0=half)
    ids = torch.cat([a[1], b[1]], 1)
    drop = torch.from_numpy(rng.random(ids.shape) < 0.1).cuda()
    ids = torch.where(drop, torch.full_like(ids, -1), ids)
    vals = torch.cat([a[0], b[0]], 1)
    cand = (vals if dtype == torch.float32 else vals.to(torch.bfloat16)).contiguous()
    got = filtered_topk(cand, k, ids=ids)
    # reference: the top k of the union of the present candidates
    ref_ids = ids.cpu().numpy()
    full = np.full((B, n), -1, dtype=np.int64)
    for d in range(B):
        present = ref_ids[d][ref_ids[d] >= 0]
        full[d, present] = present
    _same(got, ref_topk(P, k, ids=full))
    # with a filter in merge mode: candidates are tested by id
    lists = [ref_ids[d][ref_ids[d] >= 0][::3].tolist() for d in range(B)]
    flt, slots = _flt(lists, "cuda")
    _same(filtered_topk(cand, k, flt, slots=slots, ids=ids), ref_topk(P, k, ids=full, lists=lists))


def _model_params(n_ent, n_rel, rank, seed, dtype):
    return [torch.from_numpy(x).to("cuda", dtype) for x in gen.make_params(n_ent, n_rel, rank, seed)]


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sigmoid", [True, False])
def test_topk_1vN_equals_sorted_scores(sym, dtype, sigmoid):
    from r_tucker_amd import ops
    n_ent, n_rel, B, k = 5003, 11, 77, 50
    core, R, S, O = _model_params(n_ent, n_rel, (10, 64, 64), 3, dtype)
    if sym:
        O = S
    h, r = [torch.from_numpy(x).cuda() for x in gen.make_queries(n_ent, n_rel, B, 3)]
    rng = np.random.default_rng(3)
    lists = [rng.choice(n_ent, rng.integers(0, 40), replace=False).tolist() for _ in range(B)]
    flt, slots = _flt(lists, "cuda")
    flt.slots_of = lambda hh, rr: slots
    keep = torch.from_numpy(rng.integers(0, n_ent, B)).cuda()
    sdt = [torch.float32] + ([torch.bfloat16] if dtype == torch.bfloat16 and sigmoid else [])
    for score_dtype in sdt:
        P = ops.score_1vN(core, R, S, O, h, r, sigmoid=sigmoid, out_dtype=score_dtype).float().cpu().numpy()
        got = ops.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, sigmoid=sigmoid, score_dtype=score_dtype)
        _same(got, ref_topk(P, k, lists=lists, keep=keep.cpu().numpy()))
        got = ops.topk_1vN(core, R, S, O, h, r, k, sigmoid=sigmoid, score_dtype=score_dtype)
        _same(got, ref_topk(P, k))
        # entity blocks: the reference sort of the per-block score_packed_into outputs, concatenated
        nb = 1200
        _, qp = ops.query_vectors(core, R, S, h, r, packed=True)
        blocks = []
        for lo in range(0, n_ent, nb):
            out = torch.empty((B, min(nb, n_ent - lo)), dtype=score_dtype, device="cuda")
            blocks.append(ops.score_packed_into(qp, B, O[lo:lo + nb], out, sigmoid=sigmoid).float().cpu().numpy())
        Pb = np.concatenate(blocks, 1)
        got = ops.topk_1vN(core, R, S, O, h, r, k, flt=flt, keep_idx=keep, sigmoid=sigmoid, score_dtype=score_dtype,
                           entity_block=nb)
        _same(got, ref_topk(Pb, k, lists=lists, keep=keep.cpu().numpy()))


@pytest.fixture(scope="module")
def wn():
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    return data, KG_dataset(data, data.test_data, test_set=True)


def _wn_model(data, variant):
    import r_tucker_amd as rt
    n_ent, n_rel = len(data.entities), len(data.relations)
    if variant == "trained_q8":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from pack_checkpoint_q8 import dequantise
        from configs.base_config import wn18rr_readme_config
        z = np.load(os.path.join(ROOT, "tests", "golden", "wn18rr_trained_q8.npz"), allow_pickle=False)
        model = rt.AsymmetricR_TuckER((n_ent, n_rel), wn18rr_readme_config().model_cfg.manifold_rank)
        model.init()
        with torch.no_grad():
            model.core.copy_(torch.from_numpy(z["core"]))
            model.R.weight.copy_(torch.from_numpy(z["R"]))
            for n_, w in (("S", model.S.weight), ("O", model.O.weight)):
                q, r_ = torch.linalg.qr(torch.from_numpy(dequantise(z[n_ + "_q8"], z[n_ + "_scale"])).double())
                w.copy_((q * torch.sign(torch.diagonal(r_))).float())
    else:
        rank = (10, 200, 200)
        params = gen.make_params(n_ent, n_rel, rank, 322, logit_std=3.0 if variant == "spread" else 24.0)
        model = rt.AsymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": torch.from_numpy(params[0]), "R.weight": torch.from_numpy(params[1]),
                    "S.weight": torch.from_numpy(params[2]), "O.weight": torch.from_numpy(params[3])})
    return model.cuda().eval()


@pytest.mark.parametrize("variant", ["spread", "saturated", "trained_q8"])
def test_consistent_with_filtered_rank(wn, variant):
    """keep_idx = object: rank r <= k  <=>  ids[r - 1] == object; r > k: the object is not in the row."""
    import r_tucker_amd as rt
    data, ds = wn
    model = _wn_model(data, variant)
    flt = rt.DeviceFilter(ds, "cuda")
    T = rt.Tucker(model.core.data, [model.R.weight, model.S.weight, model.O.weight])
    n, k, checked = len(ds), 100, 0
    with torch.no_grad():
        for lo in range(0, n, 512):
            items = torch.arange(lo, min(lo + 512, n), device="cuda")
            f = flt.features[items]
            P = model(f[:, 0], f[:, 1])(T)
            ranks = rt.filtered_ranks(P, f[:, 2], flt, items).long()
            _, ids = rt.filtered_topk(P, k, flt, item_ids=items, keep_idx=f[:, 2])
            pt = P.gather(1, f[:, 2:3]).view(-1)
            ok = pt > 0
            inside = ranks <= k
            at = ids.gather(1, (ranks.clamp(max=k) - 1).view(-1, 1)).view(-1)
            assert bool(((at == f[:, 2]) | ~inside | ~ok).all())
            assert bool((~(ids == f[:, 2:3]).any(1) | inside | ~ok).all())
            checked += int(ok.sum())
    assert checked > 0.9 * n


@pytest.mark.parametrize("sym", [False, True])
def test_predict_with_slots_of(wn, sym):
    import r_tucker_amd as rt
    data, ds = wn
    n_ent, n_rel = len(data.entities), len(data.relations)
    rank = (10, 64, 64)
    params = gen.make_params(n_ent, n_rel, rank, 11)
    if sym:
        model = rt.SymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": torch.from_numpy(params[0]), "R.weight": torch.from_numpy(params[1]),
                    "E.weight": torch.from_numpy(params[2])})
    else:
        model = rt.AsymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": torch.from_numpy(params[0]), "R.weight": torch.from_numpy(params[1]),
                    "S.weight": torch.from_numpy(params[2]), "O.weight": torch.from_numpy(params[3])})
    model.cuda().eval()
    flt = rt.DeviceFilter(ds, "cuda")
    f = flt.features[:300]
    h = torch.cat([f[:, 0], torch.tensor([0, 1, 2], device="cuda")])
    r = torch.cat([f[:, 1], torch.tensor([n_rel - 1, 0, 3], device="cuda")])
    vals, ids = model.predict(h, r, k=20, flt=flt)
    slots = flt.slots_of(h, r)
    assert bool((slots[:300] >= 0).all())
    ptr, obj = flt.pair_ptr.cpu().numpy(), flt.pair_obj.cpu().numpy()
    idn = ids.cpu().numpy()
    for d, s in enumerate(slots.cpu().tolist()):
        if s >= 0:
            assert not np.isin(idn[d], obj[ptr[s]:ptr[s + 1]]).any()
    E = model.E.weight if sym else model.O.weight
    S = model.E.weight if sym else model.S.weight
    fltx = types.SimpleNamespace(pair_ptr=flt.pair_ptr, pair_obj=flt.pair_obj, slots_of=lambda hh, rr: slots)
    ref = rt.topk_1vN(model.core, model.R.weight, S, E, h, r, 20, flt=fltx)
    assert torch.equal(ids, ref[1]) and torch.equal(vals, ref[0])


def test_sharded_form_two_blocks():
    """Two EntityShards blocks scored and selected separately, then merged = the select of the concatenated blocks."""
    from r_tucker_amd import ops
    from r_tucker_amd.evaluation import filtered_topk
    from r_tucker_amd.sharded import EntityShards
    n_ent, n_rel, B, k = 4001, 7, 64, 30
    core, R, S, O = _model_params(n_ent, n_rel, (8, 32, 32), 4, torch.float32)
    h, r = [torch.from_numpy(x).cuda() for x in gen.make_queries(n_ent, n_rel, B, 4)]
    sh = EntityShards(n_ent, 2)
    rng = np.random.default_rng(4)
    lists = [rng.choice(n_ent, 25, replace=False).tolist() for _ in range(B)]
    flt, slots = _flt(lists, "cuda")
    blocks, parts = [], []
    for rk in range(2):
        lo, hi = sh.bounds(rk)
        Pb = ops.score_1vN(core, R, S, sh.take(O, rk), h, r)[:, : hi - lo]
        blocks.append(Pb)
        parts.append(filtered_topk(Pb, k, flt, slots=slots, col0=lo))
    merged = filtered_topk(torch.cat([p[0] for p in parts], 1), k, ids=torch.cat([p[1] for p in parts], 1))
    full = torch.cat(blocks, 1).contiguous()
    ref = filtered_topk(full, k, flt, slots=slots)
    assert torch.equal(merged[0], ref[0]) and torch.equal(merged[1], ref[1])
    _same(ref, ref_topk(full.cpu().numpy(), k, lists=lists))


def test_errors():
    from r_tucker_amd import _lib
    from r_tucker_amd.evaluation import filtered_topk
    P = torch.rand(4, 100, device="cuda")
    for k in (0, 1025):
        with pytest.raises(ValueError):
            filtered_topk(P, k)
    with pytest.raises(RuntimeError):
        filtered_topk(P.cpu(), 10)
    with pytest.raises(RuntimeError):
        filtered_topk(P.double(), 10)
    with pytest.raises(RuntimeError):
        filtered_topk(P, 10, ids=torch.zeros(4, 100, dtype=torch.int32, device="cuda"))
    lib = _lib.load()
    v = torch.empty(4, 10, device="cuda")
    i = torch.empty(4, 10, dtype=torch.int64, device="cuda")
    for k in (0, 1025):
        assert lib.rtk_select_topk_f32(P.data_ptr(), 4, 100, 100, 0, None, 0, None, None, None, None, k, v.data_ptr(),
                                       i.data_ptr(), None, 0, None) == -1
    # the select needs no workspace: the size query is 0 and a call without one is accepted
    assert lib.rtk_select_topk_workspace_bytes(4, 100, 10) == 0
    assert lib.rtk_select_topk_f32(P.data_ptr(), 4, 100, 100, 0, None, 0, None, None, None, None, 10, v.data_ptr(),
                                   i.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(i, torch.sort(P, dim=1, descending=True, stable=True)[1][:, :10])
