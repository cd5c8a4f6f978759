"""The float64 model of relation prediction (tests/relation_model.py) and the relation filter, on the CPU.

The model is tied to the pinned oracle: its z[d, r] is the oracle's 1-vs-all logit of (h_d, r) at column t_d.  Its tie
counts equal a brute-force loop, the relation filter's lists equal a dictionary built from the raw triples of
data/WN18RR, and the inputs of the GPU rank test give a float64 band whose two ends coincide for nearly every query
(otherwise that test would say nothing)."""
import os

import numpy as np
import pytest
import torch

import gen
import relation_model as rm
from oracle import score_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ["asym", "sym"])
def test_model_logits_are_the_oracles_1vN_logits(golden_meta, mode):
    c = golden_meta["cases"][f"tiny_{mode}"]
    core, R, S, O = gen.make_params(c["n_ent"], c["n_rel"], tuple(c["rank"]), c["seed"], shared=(mode == "sym"))
    h, r = gen.make_queries(c["n_ent"], c["n_rel"], c["batch"], c["seed"])
    assert gen.digest(core, R, S, O, h, r) == c["inputs_sha256"], "seeded inputs differ from the fixture's"
    rng = np.random.default_rng(5)
    t = rng.integers(0, c["n_ent"], len(h))
    z = rm.logits(core, R, S, O, h, t)                                    # (B, n_rel)
    assert z.shape == (len(h), c["n_rel"])
    for rel in range(c["n_rel"]):
        ze = orc.logits_exact(core, R, S, O, h, np.full(len(h), rel))     # (B, n_ent), float64
        ref = ze[np.arange(len(h)), t]
        assert np.max(np.abs(z[:, rel] - ref) / np.maximum(np.abs(ref), 1e-300)) <= 1e-10
    # and u itself: z = u . R^T
    u = rm.pair_vectors(core, S, O, h, t)
    assert np.allclose(u @ np.asarray(R, dtype=np.float64).T, z, rtol=1e-13, atol=0)


def test_tie_counts_equal_a_brute_force_loop():
    rng = np.random.default_rng(3)
    B, n = 60, 22
    P = rng.choice(np.array([0.0, 0.1, 0.25, 0.5, 0.5, 0.9, 1.0], dtype=np.float32), size=(B, n))   # many ties, zeros
    rel = rng.integers(0, n, B)
    known = [None if d % 5 == 0 else sorted(set(rng.integers(0, n, 4).tolist()) | {int(rel[d])}) for d in range(B)]
    for kn in (None, known):
        got = rm.tie_counts(P, rel, kn)
        want = rm.tie_counts_loop(P, rel, kn)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    g, e, before = rm.tie_counts(P, rel, known)
    assert (e > 0).any() and (g > 0).any() and np.all(before <= e)


def test_bf16_rounding_is_torchs():
    x = rm.scaled((50, 33), 1)
    assert np.array_equal(rm.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())


@pytest.fixture(scope="module")
def wn18rr():
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    return data, KG_dataset(data, data.test_data, test_set=True)


def test_relation_filter_lists_equal_the_raw_triples(wn18rr):
    from r_tucker_amd.evaluation import RelationFilter
    data, ds = wn18rr
    ei = {e: i for i, e in enumerate(data.entities)}
    ri = {r: i for i, r in enumerate(data.relations)}
    want = rm.relation_lists([(ei[s], ri[r], ei[o]) for s, r, o in data.data])      # every split, reverse triples included
    flt = RelationFilter.of(ds, "cpu")
    assert RelationFilter.of(ds, "cpu") is flt                                      # cached per dataset and device
    ptr, rel = flt.pair_ptr.numpy(), flt.pair_obj.numpy()
    assert len(ptr) - 1 == len(want) and flt.max_list == max(len(v) for v in want.values())
    keys = np.array(sorted(want), dtype=np.int64)
    slots = flt.slots_of(keys[:, 0], keys[:, 1]).numpy()
    assert sorted(slots.tolist()) == list(range(len(want)))
    for (s, o), sl in zip(sorted(want), slots.tolist()):
        assert rel[ptr[sl]:ptr[sl + 1]].tolist() == want[(s, o)]
    # the items' own slots, and pairs nobody knows
    f = np.asarray(ds.features)
    item_slots = flt.slot_of_item.numpy()
    assert np.array_equal(item_slots, flt.slots_of(f[:, 0], f[:, 2]).numpy())
    for i in range(0, len(f), 97):
        sl = item_slots[i]
        assert f[i, 1] in rel[ptr[sl]:ptr[sl + 1]]
    n_ent = len(data.entities)
    unknown = [(s, o) for s, o in [(0, 1), (5, 5), (n_ent - 1, 0), (-1, 3), (2, n_ent)] if (s, o) not in want]
    assert unknown and flt.slots_of([s for s, _ in unknown], [o for _, o in unknown]).tolist() == [-1] * len(unknown)
    assert torch.equal(flt.subj, flt.features[:, 0]) and torch.equal(flt.rel, flt.features[:, 1])
    assert torch.equal(flt.obj, flt.features[:, 2])


@pytest.mark.parametrize("n_rel", [22, 237])
def test_rank_case_band_is_not_vacuous(n_rel):
    """The inputs of tests/test_gpu_relations.py's rank test: logits with a standard deviation near 3, and a float64
    band whose ends coincide for at least 95 % of the 2000 queries at the test's own tau (twice the query's largest
    tau_p of the fp32 path)."""
    cs = rm.rank_case(n_rel)
    z, _, tau_p = rm.z_bounds(cs["core"], cs["R"], cs["S"], cs["O"], cs["h"], cs["t"], bf16=False)
    assert z.shape == (2000, n_rel) and 2.7 <= z.std() <= 3.3
    assert np.mean([len(k) for k in cs["known"]]) >= 3                  # several known relations per pair
    lo, hi = rm.band(rm.probs(z), cs["r"], cs["known"], 2 * tau_p.max(axis=1))
    share = float((lo == hi).mean())
    print(f"n_rel = {n_rel}: logit deviation {z.std():.3f}, band ends coincide for {100 * share:.1f} % of the queries")
    assert np.all(lo <= hi) and share >= 0.95
