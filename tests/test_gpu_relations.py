"""GPU tests of relation prediction, (h, ?, t): ops.score_relations against the float64 model within tau_z / tau_p
(tests/relation_model.py), its identity with the (h, r, ?) path, the id checks, the ranks of every query inside a
float64 band, the model methods and evaluate_relations against numpy on the device's own scores, and one pass over a
trained model."""
import os
import sys

import numpy as np
import pytest
import torch

import relation_model as rm
import tie_model
from oracle import score_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENT = 50


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _dev(x, bf16):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.bfloat16() if bf16 else t


def _params(a, n_rel, sym, bf16, seed, B=70, bc=20):
    core = rm.scaled((a, bc * bc), seed, -2, 2).reshape(a, bc, bc)
    R = rm.scaled((n_rel, a), seed + 1, -2, 2)
    S = rm.scaled((N_ENT, bc), seed + 2, -2, 2)
    O = S if sym else rm.scaled((N_ENT, bc), seed + 3, -2, 2)
    if bf16:
        core, R, S, O = [rm.bf16_round(x) for x in (core, R, S, O)]
    rng = np.random.default_rng(seed + 4)
    h, t, r = rng.integers(0, N_ENT, B), rng.integers(0, N_ENT, B), rng.integers(0, n_rel, B)
    return core, R, S, O, h.astype(np.int64), t.astype(np.int64), r.astype(np.int64)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("a", [10, 36])
@pytest.mark.parametrize("n_rel", [1, 22, 237])
def test_score_relations_against_float64(rt, n_rel, a, sym, bf16):
    core, R, S, O, h, t, _ = _params(a, n_rel, sym, bf16, 100 * a + n_rel)
    z64, tau_z, tau_p = rm.z_bounds(core, R, S, O, h, t, bf16)
    G, Rd, Sd = _dev(core, bf16), _dev(R, bf16), _dev(S, bf16)
    Od = Sd if sym else _dev(O, bf16)
    hd, td = torch.from_numpy(h).cuda(), torch.from_numpy(t).cuda()
    z = rt.score_relations(G, Rd, Sd, Od, hd, td, sigmoid=False)
    assert z.shape == (len(h), n_rel) and z.dtype == torch.float32
    ez = np.max(np.abs(z.cpu().numpy() - z64) / tau_z)
    print(f"n_rel={n_rel} a={a} {'sym' if sym else 'asym'} {'bf16' if bf16 else 'f32'}: max |dz| / tau_z = {ez:.2e}")
    assert ez <= 1.0
    p64 = rm.probs(z64)
    for mode in ("exact", "fast"):
        p = rt.score_relations(G, Rd, Sd, Od, hd, td, sigmoid_mode=mode)
        ep = np.max(np.abs(p.cpu().numpy() - p64) / tau_p)
        print(f"  {mode} logistic: max |dp| / tau_p = {ep:.2e}")
        assert ep <= 1.0, mode
    assert torch.equal(rt.score_relations(G, Rd, Sd, Od, hd, td, sigmoid=False), z)            # run to run
    assert torch.equal(rt.score_relations(G, Rd, Sd, Od, hd[:33], td[:33], sigmoid=False), z[:33])
    assert rt.score_relations(G, Rd, Sd, Od, hd[:0], td[:0]).shape == (0, n_rel)


def _candidate_bound(c, bf16):
    """gamma(m + 6) of rtk_score_candidates_* (include/rtucker_hip.h, tests/test_gpu_candidates.py)."""
    w = 8 if bf16 else 4
    n = w * -(-c // (64 * w)) + 6
    return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
def test_identity_with_score_triples(rt, sym, bf16):
    """score_relations(h, t)[d, r_d] is the logit score_triples(h, r_d, t_d) gives, within the sum of the two paths'
    tolerances.  The (h, r, ?) path: stage 1 within (a + b + 2) 2^-23 v_abs (tests/test_gpu_stage1_bounds.py, a <= 32),
    the candidate kernel within gamma(m + 6) sum |v| |O[t]| of its input, which in bf16 is v rounded (2^-8 relative)."""
    a, n_rel, bc = 10, 22, 20
    core, R, S, O, h, t, r = _params(a, n_rel, sym, bf16, 9)
    z64, tau_z, _ = rm.z_bounds(core, R, S, O, h, t, bf16)
    v64 = orc.query_vectors_exact(core, R, S, h, r)
    v_abs = orc.query_vectors_exact(np.abs(core), np.abs(R), np.abs(S), h, r)
    v_bound = (a + bc + 2) * 2.0 ** -23 * v_abs
    x = np.abs(np.asarray(O, dtype=np.float64)[t])
    v_in = np.abs(v64) + v_bound
    tau_t = (x * v_bound).sum(1) + _candidate_bound(bc, bf16) * (x * v_in).sum(1) * (1 + 2.0 ** -8)
    if bf16:
        tau_t += 2.0 ** -8 * (x * v_in).sum(1)
    G, Rd, Sd = _dev(core, bf16), _dev(R, bf16), _dev(S, bf16)
    Od = Sd if sym else _dev(O, bf16)
    hd, td, rd = [torch.from_numpy(i).cuda() for i in (h, t, r)]
    zr = rt.score_relations(G, Rd, Sd, Od, hd, td, sigmoid=False).cpu().numpy()[np.arange(len(h)), r]
    zt = rt.score_triples(G, Rd, Sd, Od, hd, rd, td, sigmoid=False).cpu().numpy()
    d = np.arange(len(h))
    assert np.all(np.abs(zt - z64[d, r]) <= tau_t), "the (h, r, ?) path against float64"
    err = np.max(np.abs(zr - zt) / (tau_z[d, r] + tau_t))
    print(f"{'sym' if sym else 'asym'} {'bf16' if bf16 else 'f32'}: max |z_rel - z_triple| / (tau_z + tau_triple) = {err:.2e}")
    assert err <= 1.0


def test_out_of_range_ids(rt):
    core, R, S, O, h, t, _ = _params(10, 22, False, False, 3)
    G, Rd, Sd, Od = [_dev(x, False) for x in (core, R, S, O)]
    hd, td = torch.from_numpy(h).cuda(), torch.from_numpy(t).cuda()
    good = rt.score_relations(G, Rd, Sd, Od, hd, td)
    keep = torch.arange(len(h), device="cuda") != 5
    for which, word in (("h", "subject_idx"), ("t", "object_idx")):
        h2, t2 = hd.clone(), td.clone()
        (h2 if which == "h" else t2)[5] = N_ENT
        with rt.index_check("strict"):
            with pytest.raises(IndexError, match=word):
                rt.score_relations(G, Rd, Sd, Od, h2, t2)
        with rt.index_check("deferred"):
            p = rt.score_relations(G, Rd, Sd, Od, h2, t2)
            assert torch.equal(p[keep], good[keep])
            with pytest.raises(IndexError, match=word):
                rt.check_device_errors()
    with pytest.raises(RuntimeError, match="entries"):
        rt.score_relations(G, Rd, Sd, Od, hd, td[:3])


class _TripleSet:
    """What RelationFilter and evaluate_relations read of a test-mode KG_dataset, from id triples: ``held`` (s, r, o) are
    the known triples, ``items`` the queries."""

    def __init__(self, held, items, n_ent, n_rel):
        from r_tucker_amd.data import KG_dataset
        self._pairs, self._ptr, self._obj = KG_dataset._csr(held)
        self.features = np.asarray(items, dtype=np.int64).reshape(-1, 3)
        self.n_ent, self.n_rel = n_ent, n_rel

    def __len__(self):
        return len(self.features)


def _np_topk(P, known, k):
    """numpy's selection on the device's scores: a row's known relations removed, best first, equal scores by
    ascending id, (-inf, -1) past the candidates."""
    B, n = P.shape
    vals, ids = np.full((B, k), -np.inf, dtype=np.float32), np.full((B, k), -1, dtype=np.int64)
    for d in range(B):
        cand = np.setdiff1d(np.arange(n), np.asarray(known[d] or [], dtype=np.int64))
        order = cand[np.lexsort((cand, -P[d, cand].astype(np.float64)))][:k]
        vals[d, :len(order)], ids[d, :len(order)] = P[d, order], order
    return vals, ids


@pytest.fixture(scope="module", params=[22, 237])
def rank_run(rt, request):
    """One case of relation_model.rank_case on the device: model, filter, scores and tie counts, computed once."""
    n_rel = request.param
    cs = rm.rank_case(n_rel)
    n_ent = cs["n_ent"]
    model = rt.AsymmetricR_TuckER((n_ent, n_rel), tuple(cs["core"].shape))
    with torch.no_grad():
        model.core.copy_(torch.from_numpy(cs["core"])); model.R.weight.copy_(torch.from_numpy(cs["R"]))
        model.S.weight.copy_(torch.from_numpy(cs["S"])); model.O.weight.copy_(torch.from_numpy(cs["O"]))
    model.cuda().eval()
    items = np.stack([cs["h"], cs["r"], cs["t"]], 1)
    held = sorted({(int(cs["h"][d]), int(k), int(cs["t"][d])) for d in range(len(items)) for k in cs["known"][d]})
    ds = _TripleSet(held, items, n_ent, n_rel)
    flt = rt.RelationFilter.of(ds, "cuda")
    h, r, t = [torch.from_numpy(cs[k]).cuda() for k in ("h", "r", "t")]
    P = rt.score_relations(model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data, h, t)
    greater, equal = rt.filtered_tie_counts(P, r, flt, torch.arange(len(items), device="cuda"))
    return dict(cs=cs, n_rel=n_rel, model=model, ds=ds, flt=flt, h=h, r=r, t=t, P=P, Pn=P.cpu().numpy(),
                greater=greater.cpu().numpy().astype(np.int64), equal=equal.cpu().numpy().astype(np.int64))


def test_every_rank_lies_in_the_float64_band(rt, rank_run):
    """No query left out: the device's greater and greater + equal lie in [#{p64_j > p64_t + tau}, #{p64_j >= p64_t -
    tau}] over the relations the filter leaves in, tau twice the query's largest tau_p.  The band is tight: its ends
    coincide for at least 95 % of the queries (tests/test_relation_model_host.py asserts that on these inputs)."""
    cs = rank_run["cs"]
    z64, _, tau_p = rm.z_bounds(cs["core"], cs["R"], cs["S"], cs["O"], cs["h"], cs["t"], bf16=False)
    assert np.all(np.abs(rank_run["Pn"] - rm.probs(z64)) <= tau_p)
    lo, hi = rm.band(rm.probs(z64), cs["r"], cs["known"], 2 * tau_p.max(axis=1))
    g, e = rank_run["greater"], rank_run["equal"]
    print(f"n_rel = {rank_run['n_rel']}: band ends coincide for {100 * (lo == hi).mean():.1f} % of the queries, "
          f"{int((e > 0).sum())} tied")
    assert np.all(lo <= g) and np.all(g + e <= hi)
    # the filter's slots are the queries' own lists
    assert np.array_equal(rank_run["flt"].slots_of(rank_run["h"], rank_run["t"]).cpu().numpy(),
                          rank_run["flt"].slot_of_item.cpu().numpy())


def test_ranks_topk_and_evaluation_equal_numpy_on_the_device_scores(rt, rank_run):
    cs, model, flt, ds = rank_run["cs"], rank_run["model"], rank_run["flt"], rank_run["ds"]
    h, r, t, Pn, n_rel = rank_run["h"], rank_run["r"], rank_run["t"], rank_run["Pn"], rank_run["n_rel"]
    g, e, before = rm.tie_counts(Pn, cs["r"], cs["known"])
    assert np.array_equal(rank_run["greater"], g) and np.array_equal(rank_run["equal"], e)
    stable = model.rank_relations(h, r, t, flt=flt)
    assert stable.dtype == torch.int32 and np.array_equal(stable.cpu().numpy(), 1 + g + before)
    for kind in tie_model.TYPES:
        got = model.rank_relations(h, r, t, flt=flt, rank_type=kind)
        assert np.array_equal(got.cpu().numpy(), tie_model.ranks(g, e, kind))
    g0, e0, b0 = rm.tie_counts(Pn, cs["r"], None)                                  # unfiltered
    assert np.array_equal(model.rank_relations(h, r, t).cpu().numpy(), 1 + g0 + b0)
    assert np.array_equal(model.rank_relations(h, r, t, rank_type="realistic").cpu().numpy(), tie_model.ranks(g0, e0, "realistic"))
    with pytest.raises(ValueError):
        model.rank_relations(h, r, t, rank_type="best")
    for k in (1, 3, n_rel):
        vals, ids = model.predict_relations(h, t, k=k, flt=flt)
        wv, wi = _np_topk(Pn, cs["known"], k)
        assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(vals.cpu().numpy(), wv)
    vals, ids = model.predict_relations(h[:40], t[:40], k=3)
    wv, wi = _np_topk(Pn[:40], [None] * 40, 3)
    assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(vals.cpu().numpy(), wv)
    # evaluate_relations: batches of 512; the tie-aware sums are rtk_tie_metrics_f64's, restated addition by addition
    n = len(ds)
    acc = None
    for lo in range(0, n, 512):
        acc = tie_model.metrics_sums(g[lo:lo + 512], e[lo:lo + 512], acc)
    for kind in tie_model.TYPES:
        m, loss = rt.evaluate_relations(model, ds, batch_size=512, flt=flt, rank_type=kind)
        assert loss is None and m == tie_model.metrics_of(acc, kind, n)
    m, loss = rt.evaluate_relations(model, ds, batch_size=512)                  # the cached filter of the dataset
    rs = (1 + g + before).astype(np.float64)
    assert loss is None and sorted(m) == ["hits@1", "hits@10", "hits@3", "mrr"]
    for k in (1, 3, 10):
        assert m[f"hits@{k}"] == (rs <= k).sum() / n
    assert abs(m["mrr"] - (1.0 / rs).mean()) <= 1e-12                          # float64 sums in another order


def test_trained_model_relations():
    """evaluate_relations over the first 512 test triples of WN18RR on the trained fixture: runs clean, and its metrics
    are numpy's on the device's tie counts.  The metrics are printed; no value is required of them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import r_tucker_amd as rt
    from configs.base_config import wn18rr_readme_config
    from pack_checkpoint_q8 import dequantise
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    rank = wn18rr_readme_config().model_cfg.manifold_rank
    model = rt.AsymmetricR_TuckER((len(data.entities), len(data.relations)), rank)
    model.init()
    z = np.load(os.path.join(ROOT, "tests", "golden", "wn18rr_trained_q8.npz"), allow_pickle=False)
    with torch.no_grad():
        model.core.copy_(torch.from_numpy(z["core"]))
        model.R.weight.copy_(torch.from_numpy(z["R"]))
        for n_, w in zip(("S", "O"), (model.S.weight, model.O.weight)):
            q, r_ = torch.linalg.qr(torch.from_numpy(dequantise(z[n_ + "_q8"], z[n_ + "_scale"])).double())
            w.copy_((q * torch.sign(torch.diagonal(r_))).float())
    model.cuda()
    ds = KG_dataset(data, data.test_data[:512], test_set=True)
    flt = rt.RelationFilter.of(ds, "cuda")
    out = {}
    for kind in (None,) + tie_model.TYPES:
        out[kind or "stable"], loss = rt.evaluate_relations(model, ds, batch_size=512, rank_type=kind)
        assert loss is None
    print("\nrelation prediction, first 512 WN18RR test triples:", out)
    f = flt.features
    P = rt.score_relations(model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data, f[:, 0], f[:, 2])
    ids = torch.arange(len(ds), device="cuda")
    greater, equal = rt.filtered_tie_counts(P, f[:, 1], flt, ids)
    ranks = rt.filtered_ranks(P, f[:, 1], flt, ids).cpu().numpy().astype(np.float64)
    rt.check_device_errors()
    assert np.isfinite(P.cpu().numpy()).all() and P.shape == (512, len(data.relations))
    acc = tie_model.metrics_sums(greater.cpu().numpy(), equal.cpu().numpy())
    for kind in tie_model.TYPES:
        assert out[kind] == tie_model.metrics_of(acc, kind, 512)
    for k in (1, 3, 10):
        assert out["stable"][f"hits@{k}"] == (ranks <= k).sum() / 512
    assert abs(out["stable"]["mrr"] - (1.0 / ranks).mean()) <= 1e-12
    lo, hi = 1 + greater.cpu().numpy(), 1 + (greater + equal).cpu().numpy()
    assert np.all(lo <= ranks) and np.all(ranks <= hi)
