"""The tie-aware rank counts without a GPU: the numpy model of the semantics (tests/tie_model.py) on the engineered tie
fixture and against every rank the reference recorded on the WN18RR fixtures, and the Python helpers
(``ranks_from_tie_counts``, ``metrics_from_tie_counts``, the refusals of ``rank_1vN(rank_type=...)``).

The interval test is the statement the project can make about a tied target whatever the host: every recorded reference
rank lies in [1 + greater, 1 + greater + equal] (the reference's unstable CPU sort picks some place in the tie block),
with no query allowed outside."""
import os

import numpy as np
import pytest
import torch

import gen
import tie_model
from oracle import score_oracle as orc

import r_tucker_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engineered_ties(golden):
    z = golden("ties")
    P, t, o = z["P"], z["t"], z["o"].reshape(-1)
    gt, eq, before = tie_model.tie_counts(P, o, known=t)
    np.testing.assert_array_equal(gt, [1, 0, 0])
    np.testing.assert_array_equal(eq, [1, 4, 1])
    assert (eq > 0).all() and eq.max() == 4
    stable = orc.filter_and_rank_stable(torch.from_numpy(P), torch.from_numpy(t), torch.from_numpy(o)).numpy()
    np.testing.assert_array_equal(stable, 1 + gt + before)
    assert ((1 + gt <= z["ranks"]) & (z["ranks"] <= 1 + gt + eq)).all()      # the reference's own ranks
    # the same from per-query lists of ids, and block by block
    lists = [np.nonzero(row)[0].tolist() for row in t]
    for a, b in zip(tie_model.tie_counts(P, o, known=lists), (gt, eq, before)):
        np.testing.assert_array_equal(a, b)
    pt = P[np.arange(3), o]
    parts = [tie_model.tie_counts(P[:, lo:hi], o, known=lists, col0=lo, pt=pt) for lo, hi in ((0, 2), (2, 5), (5, 6))]
    for k, whole in enumerate((gt, eq, before)):
        np.testing.assert_array_equal(sum(p[k] for p in parts), whole)


def test_model_special_values():
    nan, inf = float("nan"), float("inf")
    P = np.array([[nan, 1.0, nan, 0.5],          # NaN target: 0, 0
                  [0.5, nan, 0.5, inf],          # NaN competitors never count
                  [-0.0, 0.0, 0.3, 0.0],         # -0 == +0
                  [0.0, 0.7, 0.2, 0.0]],         # a filtered object joins the zeros
                 dtype=np.float32)
    obj = np.array([0, 0, 0, 0])
    gt, eq, before = tie_model.tie_counts(P, obj, known=[None, None, None, [1, 0, 9]])
    np.testing.assert_array_equal(gt, [0, 1, 1, 1])
    np.testing.assert_array_equal(eq, [0, 1, 2, 2])
    np.testing.assert_array_equal(before, [0, 0, 0, 0])


@pytest.fixture(scope="module")
def wn():
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    return data, {"valid": KG_dataset(data, data.valid_data, test_set=True),
                  "test": KG_dataset(data, data.test_data, test_set=True)}


@pytest.mark.parametrize("variant,logit_std", [("saturated", 24.0), ("spread", 3.0)])
def test_reference_ranks_lie_in_the_tie_interval(wn, golden, golden_meta, variant, logit_std):
    data, ds = wn
    n_ent, n_rel, rank, seed = len(data.entities), len(data.relations), (10, 200, 200), 322
    params = gen.make_params(n_ent, n_rel, rank, seed, logit_std=logit_std)
    core, R, S, O = [torch.from_numpy(x) for x in params]
    g = golden("wn18rr_rank")
    for split in ("valid", "test"):
        assert gen.digest(*params) == golden_meta["cases"][f"rank_{variant}_{split}"]["inputs_sha256"]
        d = ds[split]
        ref = g[f"{variant}_{split}_ranks"].astype(np.int64)
        assert len(ref) == len(d)
        gts, eqs = [], []
        for lo in range(0, len(d), 512):                 # the batches the reference ranked
            ids = np.arange(lo, min(lo + 512, len(d)))
            f = torch.from_numpy(d.features[ids])
            P = orc.score_ref(core, R, S, O, f[:, 0], f[:, 1]).numpy()
            gt, eq, _ = tie_model.tie_counts(P, f[:, 2].numpy(), known=d.dense_targets(ids).numpy())
            gts.append(gt)
            eqs.append(eq)
        gt, eq = np.concatenate(gts), np.concatenate(eqs)
        outside = int(((ref < 1 + gt) | (ref > 1 + gt + eq)).sum())
        tied = int((eq > 0).sum())
        print(f"\n{variant}/{split}: {len(d)} queries, {tied} tied (largest tie block {int(eq.max())}), "
              f"{outside} reference ranks outside [1 + greater, 1 + greater + equal]")
        assert outside == 0
        if (variant, split) == ("saturated", "valid"):
            assert tied >= 2000                          # the interval is not a point here: the test is not vacuous


def test_ranks_from_tie_counts():
    rng = np.random.default_rng(0)
    g, e = rng.integers(0, 50000, 300), rng.integers(0, 20000, 300) * (rng.random(300) < 0.5)
    tg, te = torch.from_numpy(g).to(torch.int32), torch.from_numpy(e).to(torch.int32)
    for name in tie_model.TYPES:
        got = rt.ranks_from_tie_counts(tg, te, name)
        assert got.dtype == torch.float64
        np.testing.assert_array_equal(got.numpy(), tie_model.ranks(g, e, name))
    np.testing.assert_array_equal(rt.ranks_from_tie_counts(tg, te, "realistic").numpy(), 1 + g + e / 2)
    for bad in ("stable", "average", None):
        with pytest.raises(ValueError, match="optimistic"):
            rt.ranks_from_tie_counts(tg, te, bad)


def test_metrics_from_tie_counts():
    rng = np.random.default_rng(1)
    g, e = rng.integers(0, 12, 500), rng.integers(0, 5, 500)
    m = rt.metrics_from_tie_counts(torch.from_numpy(g).to(torch.int32), torch.from_numpy(e).to(torch.int32))
    acc = tie_model.metrics_sums(g, e)
    for k, name in enumerate(tie_model.TYPES):
        r = tie_model.ranks(g, e, name)
        assert float(m[name]["mrr"]) == pytest.approx(float((1.0 / r).sum()), rel=1e-14)
        assert acc[4 * k] == pytest.approx(float((1.0 / r).sum()), rel=1e-14)      # (another order of additions)
        for j, top in enumerate((1, 3, 10)):
            assert int(m[name][f"hits@{top}"]) == int((r <= top).sum()) == int(acc[4 * k + 1 + j])
    assert int(m["tied"]) == int((e > 0).sum()) == int(acc[12])
    assert m["optimistic"]["mrr"] >= m["realistic"]["mrr"] >= m["pessimistic"]["mrr"]
    # the sums ADD to the accumulators, batch by batch
    both = tie_model.metrics_sums(g[300:], e[300:], tie_model.metrics_sums(g[:300], e[:300]))
    np.testing.assert_allclose(both, acc, rtol=1e-14)


def _model(sym):
    model = (rt.SymmetricR_TuckER if sym else rt.AsymmetricR_TuckER)((20, 3), (2, 4, 4))
    model.init()
    return model


def _factors(model, sym):
    return (model.core, model.R.weight) + ((model.E.weight, model.E.weight) if sym else (model.S.weight, model.O.weight))


@pytest.mark.parametrize("sym", [False, True])
def test_rank_type_refusals(sym):
    model = _model(sym)
    h, r, t = torch.tensor([1, 2]), torch.tensor([0, 1]), torch.tensor([3, 4])
    ops = _factors(model, sym)
    for call in (lambda **kw: rt.rank_1vN(*ops, h, r, t, **kw), lambda **kw: model.rank_objects(h, r, t, **kw)):
        with pytest.raises(ValueError) as ei:
            call(rank_type="average")
        for name in ("stable", "optimistic", "realistic", "pessimistic"):
            assert name in str(ei.value)
        with pytest.raises(ValueError, match="want_bce"):
            call(rank_type="realistic", want_bce=True)
    with pytest.raises(ValueError, match="optimistic"):
        rt.evaluate(model, [], rank_type="stable")


@pytest.mark.parametrize("sym", [False, True])
def test_refuse_cpu_tensors(sym):
    model = _model(sym)
    h, r, t = torch.tensor([1, 2]), torch.tensor([0, 1]), torch.tensor([3, 4])
    ops = _factors(model, sym)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.rank_ties_1vN(*ops, h, r, t)
    for name in tie_model.TYPES:
        with pytest.raises(RuntimeError, match="no CPU path"):
            rt.rank_1vN(*ops, h, r, t, rank_type=name)
        with pytest.raises(RuntimeError, match="no CPU path"):
            model.rank_objects(h, r, t, rank_type=name)
    qp = torch.zeros(4096, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.rank_tie_counts_block_1vN(qp, 2, ops[3], 0, 20, torch.zeros(2), t)
    P = torch.rand(2, 20)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.filtered_tie_counts(P, t)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.tie_counts_block(P, t, 0, torch.zeros(2))


@pytest.mark.parametrize("sym", [False, True])
def test_object_idx_length_checked(sym):
    model = _model(sym)
    h, r = torch.tensor([1, 2]), torch.tensor([0, 1])
    ops = _factors(model, sym)
    with pytest.raises(RuntimeError, match="object_idx has 3 entries for 2 queries"):
        rt.rank_ties_1vN(*ops, h, r, torch.tensor([3, 4, 5]))
    with pytest.raises(RuntimeError, match="object_idx has 1 entries for 2 queries"):
        rt.rank_1vN(*ops, h, r, torch.tensor([3]), rank_type="pessimistic")
    with pytest.raises(RuntimeError, match="object_idx has 3 entries for 2 queries"):
        model.rank_objects(h, r, torch.tensor([3, 4, 5]), rank_type="optimistic")
