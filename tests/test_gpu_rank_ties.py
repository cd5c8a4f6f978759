"""GPU tests of the tie-aware rank counts: matrix-free (ops.rank_ties_1vN / rank_tie_counts_block_1vN,
rtk_score_rank_tie_counts_*), stored form (evaluation.filtered_tie_counts / tie_counts_block,
rtk_filtered_tie_counts_partial_f32), the metric sums (rtk_tie_metrics_f64) and evaluate(rank_type=...).

The counts are integers, so every check is exact.  The reference is the numpy model of the semantics
(tests/tie_model.py) applied to the probabilities the stored score kernels write -- for fp32 operands the ws kernel's,
for bf16 operands rtk_score_packed_bf16's (tests/test_gpu_rank.py::_stored_scores) -- with the same packed query planes,
flags and filter.  The metric sums are compared for equality with the model's restatement of the kernel's additions."""
import os
import sys

import numpy as np
import pytest
import torch

import gen
import tie_model
from test_gpu_rank import Flt, _filter, _flags, _problem, _stored_scores

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _lists(flt):
    """The per-query lists of global ids behind a filter stand-in (None: the query has no list)."""
    if flt is None:
        return None
    ptr, obj, slots = [x.cpu().numpy() for x in (flt.pair_ptr, flt.pair_obj, flt.slot_of_item)]
    return [obj[ptr[s]:ptr[s + 1]].tolist() if s >= 0 else None for s in slots]


def _check_case(rt, core, R, S, O, h, r, t, flt, mode):
    """rank_ties_1vN == the model on the stored probabilities, with and without the filter; the bracket around the
    stable rank; rank_1vN(rank_type=...).  Returns the stored probabilities and the filtered counts."""
    B = h.numel()
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, B, O, _flags(rt, mode)).cpu().numpy()
    tn = t.cpu().numpy()
    for f in (None, flt):
        gt, eq, before = tie_model.tie_counts(P, tn, known=_lists(f))
        g, e = rt.rank_ties_1vN(core, R, S, O, h, r, t, flt=f, sigmoid_mode=mode)
        assert g.dtype == torch.int32 and e.dtype == torch.int32 and g.shape == (B,) and e.shape == (B,)
        np.testing.assert_array_equal(g.cpu().numpy(), gt)
        np.testing.assert_array_equal(e.cpu().numpy(), eq)
        stable = rt.rank_1vN(core, R, S, O, h, r, t, flt=f, sigmoid_mode=mode).cpu().numpy()
        assert ((1 + gt <= stable) & (stable <= 1 + gt + eq)).all()
        np.testing.assert_array_equal(stable, 1 + gt + before)
        untied = eq == 0
        assert (stable[untied] == 1 + gt[untied]).all()            # all three rank types and the stable rank agree
        for name in tie_model.TYPES:
            got = rt.rank_1vN(core, R, S, O, h, r, t, flt=f, sigmoid_mode=mode, rank_type=name)
            assert got.dtype == torch.float64
            assert torch.equal(got, rt.ranks_from_tie_counts(g, e, name))
            np.testing.assert_array_equal(got.cpu().numpy(), tie_model.ranks(gt, eq, name))
    return P, gt, eq


SHAPES_F32 = [
    # (N, c, B, gain)
    (100, 4, 5, 1.0),             # KS = 1
    (20, 8, 33, 40.0),            # fewer entities than one tile
    (333, 36, 70, 40.0),          # KS = 3, N % 32 != 0, three query tiles
    (167, 208, 96, 1.0),          # KS = 13
    (2000, 200, 64, 1.0),
    (5000, 200, 300, 40.0),       # 40 entity tiles, ragged last query tile; saturated
]


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B,gain", SHAPES_F32)
def test_f32_tie_counts_equal_model(rt, N, c, B, gain, mode):
    core, R, S, O, h, r, t = _problem(N, c, B, N + c, gain)
    P, gt, eq = _check_case(rt, core, R, S, O, h, r, t, _filter(N, t, N), mode)
    if gain > 1.0:
        assert (P == 1.0).mean() > 0.05                             # the tie-heavy case is really tie heavy
        assert (eq > 0).any()


def test_f32_tie_counts_wn18rr_shape(rt):
    N, c, B, gain = 40943, 200, 500, 40.0
    core, R, S, O, h, r, t = _problem(N, c, B, N + c, gain)
    P, gt, eq = _check_case(rt, core, R, S, O, h, r, t, _filter(N, t, N), "exact")
    assert (P == 1.0).mean() > 0.05
    assert eq.max() > 1000                                          # tie blocks of thousands: past 16 bits per slot


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B", [(777, 18, 70), (500, 72, 33), (3000, 512, 96)])
def test_bf16_tie_counts_equal_model(rt, N, c, B, mode):
    core, R, S, O, h, r, t = _problem(N, c, B, c, 8.0, dtype=torch.bfloat16, shared=True)
    _check_case(rt, core, R, O, O, h, r, t, _filter(N, t, c), mode)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_zero_target_scores(rt, mode):
    """Targets on a row minimum that is exactly 0.0, with filter lists inside the block: a filtered object becomes a
    0 and joins `equal` (the `0 == pt` correction of the filter pass)."""
    N, c, B = 333, 36, 70
    core, R, S, O, h, r, _ = _problem(N, c, B, 77, 2000.0)
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, B, O, _flags(rt, mode))
    t = P.argmin(dim=1)
    pt = P[torch.arange(B).cuda(), t]
    assert (pt == 0.0).all()
    flt = _filter(N, t, 77)
    lists = _lists(flt)
    Pn, tn = P.cpu().numpy(), t.cpu().numpy()
    moved = [sum(1 for g in (l or []) if 0 <= g < N and g != tn[d] and Pn[d, g] != 0.0) for d, l in enumerate(lists)]
    assert sum(1 for l in lists if l) > B // 4 and sum(moved) > 0   # non-empty lists in the block; some entries move
    _, gt, eq = _check_case(rt, core, R, S, O, h, r, t, flt, mode)
    gt0, eq0, _ = tie_model.tie_counts(Pn, tn)
    np.testing.assert_array_equal(eq - eq0, moved)                  # every moved entry is one more equal ...
    np.testing.assert_array_equal(gt0 - gt, moved)                  # ... and one fewer greater


def _hand_built():
    nan, inf = float("nan"), float("inf")
    B, N = 5, 300
    rng = np.random.default_rng(4)
    P = rng.random((B, N)).astype(np.float32)
    obj = np.array([7, 150, 299, 130, 0], dtype=np.int64)
    P[0, 7] = nan                                                   # NaN target: 0, 0
    P[0, [3, 200]] = nan
    P[1, 150] = 0.5                                                 # NaN competitors, +inf, equals on both sides
    P[1, [1, 149, 151, 298]] = [nan, 0.5, 0.5, 0.5]
    P[1, [20, 290]] = [inf, nan]
    P[2, 299] = -0.0                                                # -0 == +0; listed objects join the zeros
    P[2, [0, 5, 117, 118]] = [0.0, -0.0, 0.0, -0.0]
    P[3, :] = 0.25                                                  # a row of all-equal values
    P[4, 0] = inf                                                   # +inf target
    P[4, [116, 117, 256]] = inf
    lists = [[3, 9, 7], [149, 20, 298, 30], [10, 11, 117, 299], [130, 0, 129, 131, 299, -3, N, N + 5], [117, 1, 0]]
    return P, obj, lists


def test_stored_form_equals_model(rt):
    P, obj, lists = _hand_built()
    B, N = P.shape
    flt = Flt(lists, np.arange(B))
    Pd, od, ids = torch.from_numpy(P).cuda(), torch.from_numpy(obj).cuda(), torch.arange(B).cuda()
    for f, known in ((None, None), (flt, lists)):
        gt, eq, before = tie_model.tie_counts(P, obj, known=known)
        g, e = rt.filtered_tie_counts(Pd, od, f, ids if f is not None else None)
        assert g.dtype == torch.int32 and e.dtype == torch.int32
        np.testing.assert_array_equal(g.cpu().numpy(), gt)
        np.testing.assert_array_equal(e.cpu().numpy(), eq)
        stable = rt.filtered_ranks(Pd, od, f, ids if f is not None else None).cpu().numpy()
        np.testing.assert_array_equal(stable, 1 + gt + before)
        assert gt[0] == 0 and eq[0] == 0                            # the NaN target
        assert eq[3] == (N - 1 if f is None else N - 5)             # the all-equal row; 4 listed others became 0
        # blocks of columns (views into P: the row pitch is not the block width), the target scores completed first
        pt = torch.stack([rt.evaluation.target_scores_block(Pd[:, lo:hi], od, lo) for lo, hi in ((0, 117), (117, N))]).max(0).values
        parts = [rt.tie_counts_block(Pd[:, lo:hi], od, lo, pt, f, ids if f is not None else None)
                 for lo, hi in ((0, 117), (117, N))]
        np.testing.assert_array_equal((parts[0][0] + parts[1][0]).cpu().numpy(), gt)
        np.testing.assert_array_equal((parts[0][1] + parts[1][1]).cpu().numpy(), eq)
    e0 = torch.zeros(0, dtype=torch.int64).cuda()
    g, e = rt.filtered_tie_counts(Pd[:0], e0)
    assert g.shape == (0,) and e.shape == (0,) and g.dtype == torch.int32


def test_partition_invariance_and_determinism(rt):
    N, c, B = 5000, 200, 300
    core, R, S, O, h, r, t = _problem(N, c, B, 5, 40.0)
    flt = _filter(N, t, 5)
    slots = flt.slot_of_item
    g, e = rt.rank_ties_1vN(core, R, S, O, h, r, t, flt=flt)
    g2, e2 = rt.rank_ties_1vN(core, R, S, O, h, r, t, flt=flt)
    assert torch.equal(g, g2) and torch.equal(e, e2)
    assert (e > 0).any()
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    # a block edge inside a 128-row tile; two even halves
    for blocks in (((0, 117), (117, 1000), (1000, N)), ((0, N // 2), (N // 2, N))):
        pt = torch.stack([rt.rank_targets_block(qp, B, O[lo:hi], lo, N, t) for lo, hi in blocks]).max(dim=0).values
        parts = [rt.rank_tie_counts_block_1vN(qp, B, O[lo:hi], lo, N, pt, t, flt=flt, slots=slots) for lo, hi in blocks]
        assert torch.equal(sum(p[0] for p in parts), g) and torch.equal(sum(p[1] for p in parts), e)
        parts = [rt.rank_tie_counts_block_1vN(qp, B, O[lo:hi], lo, N, pt, t) for lo, hi in blocks]
        g0, e0 = rt.rank_ties_1vN(core, R, S, O, h, r, t)
        assert torch.equal(sum(p[0] for p in parts), g0) and torch.equal(sum(p[1] for p in parts), e0)
    # a query's counts do not depend on its batch or its place in it
    parts = []
    for lo, hi in ((0, 117), (117, B)):
        flt.slot_of_item = slots[lo:hi]
        parts.append(rt.rank_ties_1vN(core, R, S, O, h[lo:hi], r[lo:hi], t[lo:hi], flt=flt))
    assert torch.equal(torch.cat([p[0] for p in parts]), g) and torch.equal(torch.cat([p[1] for p in parts]), e)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(B)).cuda()
    flt.slot_of_item = slots[perm]
    gp, ep = rt.rank_ties_1vN(core, R, S, O, h[perm], r[perm], t[perm], flt=flt)
    assert torch.equal(gp, g[perm]) and torch.equal(ep, e[perm])


def test_errors_and_edges(rt):
    N, c, B = 300, 32, 40
    core, R, S, O, h, r, t = _problem(N, c, B, 9)
    bad = t.clone()
    bad[3] = N
    with rt.index_check("deferred"):
        rt.rank_ties_1vN(core, R, S, O, h, r, bad)
        with pytest.raises(IndexError, match="object_idx"):
            rt.check_device_errors()
        rt.rank_1vN(core, R, S, O, h, r, bad, rank_type="pessimistic")
        with pytest.raises(IndexError, match="object_idx"):
            rt.check_device_errors()
        rt.check_device_errors()                     # the word was cleared
    with pytest.raises(IndexError):                  # strict (default): raised by the call itself
        rt.rank_ties_1vN(core, R, S, O, h, r, bad)
    with pytest.raises(IndexError):
        rt.rank_1vN(core, R, S, O, h, r, bad, rank_type="optimistic")
    e = torch.zeros(0, dtype=torch.int64).cuda()
    g0, e0 = rt.rank_ties_1vN(core, R, S, O, e, e, e)
    assert g0.shape == (0,) and e0.shape == (0,) and g0.dtype == torch.int32 and e0.dtype == torch.int32
    out = rt.rank_1vN(core, R, S, O, e, e, e, rank_type="realistic")
    assert out.shape == (0,) and out.dtype == torch.float64
    # N = 1: nothing but the target
    core1, R1, S1, O1, h1, r1, _ = _problem(1, c, 7, 3)
    t1 = torch.zeros(7, dtype=torch.int64).cuda()
    g1, e1 = rt.rank_ties_1vN(core1, R1, S1, O1, h1, r1, t1)
    assert not g1.any() and not e1.any()
    with pytest.raises(RuntimeError, match="above 208"):
        core2, R2, S2, O2, h2, r2, t2 = _problem(50, 224, 4, 1)
        rt.rank_ties_1vN(core2, R2, S2, O2, h2, r2, t2)


@pytest.mark.parametrize("sym", [False, True])
def test_model_rank_objects_rank_type(rt, sym):
    n_ent, n_rel, rank = 900, 5, (4, 48, 48)
    params = [torch.from_numpy(x) for x in gen.make_params(n_ent, n_rel, rank, 11, shared=sym)]
    h, r = [torch.from_numpy(x).cuda() for x in gen.make_queries(n_ent, n_rel, 70, 11)]
    t = torch.from_numpy(np.random.default_rng(11).integers(0, n_ent, 70)).cuda()
    if sym:
        model = rt.SymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": params[0], "R.weight": params[1], "E.weight": params[2]})
        S = O = model.cuda().E.weight
    else:
        model = rt.AsymmetricR_TuckER((n_ent, n_rel), rank)
        model.init({"core": params[0], "R.weight": params[1], "S.weight": params[2], "O.weight": params[3]})
        model.cuda()
        S, O = model.S.weight, model.O.weight
    model.eval()
    flt = _filter(n_ent, t, 11)
    g, e = rt.rank_ties_1vN(model.core, model.R.weight, S, O, h, r, t, flt=flt)
    for name in tie_model.TYPES:
        got = model.rank_objects(h, r, t, flt=flt, rank_type=name)
        assert got.dtype == torch.float64 and torch.equal(got, rt.ranks_from_tie_counts(g, e, name))
    assert torch.equal(model.rank_objects(h, r, t, flt=flt, rank_type="stable"), model.rank_objects(h, r, t, flt=flt))


def test_tie_metrics_kernel_equals_model(rt):
    """rtk_tie_metrics_f64 adds to its 13 accumulators exactly what the model's restatement of its additions gives."""
    lib = rt._lib.load()
    rng = np.random.default_rng(2)
    acc = torch.zeros(13, dtype=torch.float64).cuda()
    want = np.zeros(13)
    for B in (1, 70, 256, 1000):
        g = rng.integers(0, 40000, B) * (rng.random(B) < 0.7)
        e = rng.integers(0, 15000, B) * (rng.random(B) < 0.5)
        gd, ed = torch.from_numpy(g).to(torch.int32).cuda(), torch.from_numpy(e).to(torch.int32).cuda()
        rt._lib.check(lib.rtk_tie_metrics_f64(gd.data_ptr(), ed.data_ptr(), B, acc.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "rtk_tie_metrics_f64")
        want = tie_model.metrics_sums(g, e, want)
        np.testing.assert_array_equal(acc.cpu().numpy(), want)
        m = rt.metrics_from_tie_counts(gd, ed)
        batch = tie_model.metrics_sums(g, e)
        for k, name in enumerate(tie_model.TYPES):
            assert [int(m[name][f"hits@{top}"]) for top in (1, 3, 10)] == [int(x) for x in batch[4 * k + 1:4 * k + 4]]
        assert int(m["tied"]) == int(batch[12])


@pytest.fixture(scope="module")
def wn():
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    return data, {"valid": KG_dataset(data, data.valid_data, test_set=True),
                  "test": KG_dataset(data, data.test_data, test_set=True)}


def _trained_model(rt, data):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from configs.base_config import wn18rr_readme_config
    from pack_checkpoint_q8 import dequantise
    rank = wn18rr_readme_config().model_cfg.manifold_rank
    model = rt.AsymmetricR_TuckER((len(data.entities), len(data.relations)), rank)
    model.init()
    z = np.load(os.path.join(ROOT, "tests", "golden", "wn18rr_trained_q8.npz"), allow_pickle=False)
    with torch.no_grad():
        model.core.copy_(torch.from_numpy(z["core"]))
        model.R.weight.copy_(torch.from_numpy(z["R"]))
        for n, w in (("S", model.S.weight), ("O", model.O.weight)):
            q, r_ = torch.linalg.qr(torch.from_numpy(dequantise(z[n + "_q8"], z[n + "_scale"])).double())
            w.copy_((q * torch.sign(torch.diagonal(r_))).float())
    return model


def _saturated_model(rt, data):
    n_ent, n_rel = len(data.entities), len(data.relations)
    params = gen.make_params(n_ent, n_rel, (10, 200, 200), 322, logit_std=24.0)
    model = rt.AsymmetricR_TuckER((n_ent, n_rel), (10, 200, 200))
    model.init({"core": torch.from_numpy(params[0]), "R.weight": torch.from_numpy(params[1]),
                "S.weight": torch.from_numpy(params[2]), "O.weight": torch.from_numpy(params[3])})
    return model


@pytest.mark.parametrize("which,split", [("trained", "test"), ("saturated", "valid")])
def test_evaluate_rank_type(rt, wn, which, split):
    """evaluate(rank_type=...) returns the metrics of the numpy model's sums over the per-batch counts (equal, not
    close), leaves evaluate() as it was, and brackets the stable rule's MRR."""
    data, ds = wn
    model = (_trained_model if which == "trained" else _saturated_model)(rt, data).cuda().eval()
    d = ds[split]
    n = len(d)
    flt = rt.DeviceFilter(d, "cuda")
    before = rt.evaluate(model, d, batch_size=512, flt=flt)
    got = {name: rt.evaluate(model, d, batch_size=512, flt=flt, rank_type=name) for name in tie_model.TYPES}
    after = rt.evaluate(model, d, batch_size=512, flt=flt)
    assert before == after                                           # rank_type=None: the same numbers, bit for bit
    assert set(before[0]) == {"mrr", "hits@1", "hits@3", "hits@10"}
    # the counts batch by batch on the scores evaluate() ranks, against the numpy model; their sums in the kernel's order
    T = rt.Tucker(model.core.data, [model.R.weight, model.S.weight, model.O.weight])
    acc = np.zeros(13)
    stable_sum = 0.0
    with torch.no_grad():
        for lo in range(0, n, 512):
            ids = np.arange(lo, min(lo + 512, n))
            idd = torch.from_numpy(ids).cuda()
            f = flt.features[idd]
            P = model(f[:, 0], f[:, 1])(T)
            g, e = rt.filtered_tie_counts(P, f[:, 2], flt, idd)
            gt, eq, bf = tie_model.tie_counts(P.cpu().numpy(), f[:, 2].cpu().numpy(), known=d.dense_targets(ids).numpy())
            np.testing.assert_array_equal(g.cpu().numpy(), gt)
            np.testing.assert_array_equal(e.cpu().numpy(), eq)
            stable = rt.filtered_ranks(P, f[:, 2], flt, idd).cpu().numpy()
            np.testing.assert_array_equal(stable, 1 + gt + bf)
            stable_sum += float((1.0 / stable).sum())
            acc = tie_model.metrics_sums(gt, eq, acc)
    assert abs(stable_sum / n - before[0]["mrr"]) < 1e-12           # these ARE the scores evaluate() ranked
    for name in tie_model.TYPES:
        metrics, loss = got[name]
        assert metrics == tie_model.metrics_of(acc, name, n), name
        assert loss == before[1]
    mrr = {name: got[name][0]["mrr"] for name in tie_model.TYPES}
    assert mrr["optimistic"] >= before[0]["mrr"] >= mrr["pessimistic"]
    assert mrr["optimistic"] >= mrr["realistic"] >= mrr["pessimistic"]
    tied = got["realistic"][0]["tied"]
    print(f"\n{which}/{split}: {n} queries, tied {tied:.4f}; MRR optimistic {mrr['optimistic']:.5f}, stable "
          f"{before[0]['mrr']:.5f}, realistic {mrr['realistic']:.5f}, pessimistic {mrr['pessimistic']:.5f}")
    if which == "saturated":
        assert tied > 0.25                                           # a tie-dominated evaluation says so
        # the loop through the model's closure and the driver's pass-through give the same metrics
        from r_tucker_amd import driver, evaluation
        dev = torch.device("cuda", torch.cuda.current_device())
        assert evaluation._evaluate_generic(model, d, 512, dev, flt, "realistic")[0] == got["realistic"][0]
        assert evaluation._evaluate_generic(model, d, 512, dev, flt)[0] == before[0]
        assert driver.evaluate(model, d, 512, flt, rank_type="pessimistic") == got["pessimistic"]
        assert driver.evaluate(model, d, 512, flt) == before
