"""GPU tests of filtered ranking without the score matrix (ops.rank_1vN, rtk_score_rank_*, csrc/rtk_score_rank.hip).

Ranks are integers, so the checks are exact: they must equal rtk_filtered_rank_f32 (evaluation.filtered_ranks) over
the scores the stored kernels write -- for fp32 operands the ws kernel's (RTK_SCORE_KERNEL_WS), for bf16 operands
rtk_score_packed_bf16's -- with the same packed query planes, flags and filter."""
import os

import numpy as np
import pytest
import torch

import gen
from oracle import score_oracle as orc

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
        self.pair_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64).cuda()
        self.pair_obj = torch.tensor(np.concatenate([np.asarray(x, dtype=np.int64) for x in lists] + [np.zeros(0, np.int64)]),
                                     dtype=torch.int64).cuda()
        self.slot_of_item = torch.as_tensor(slots, dtype=torch.int64).cuda()

    def slots_of(self, h, r):
        return self.slot_of_item


def _flags(rt, mode):
    L = rt._lib
    return L.RTK_SCORE_SIGMOID | (L.RTK_SCORE_SIGMOID_FAST if mode == "fast" else 0)


def _stored_scores(rt, qp, B, O, flags):
    """(B, N) fp32 probabilities from the stored score kernel: fp32 operands through the ws kernel, bf16 through
    rtk_score_packed_bf16."""
    lib = rt._lib.load()
    O = O.contiguous()                    # (a factor copied from a QR result can be column-major)
    N, c = O.shape
    P = torch.empty((B, N), dtype=torch.float32, device=O.device)
    sp = torch.cuda.current_stream().cuda_stream
    if O.dtype == torch.bfloat16:
        rt._lib.check(lib.rtk_score_packed_bf16(qp.data_ptr(), B, c, O.data_ptr(), N, P.data_ptr(), N, flags, sp), "bf16")
    else:
        rt._lib.check(lib.rtk_score_packed_f32(qp.data_ptr(), B, c, O.data_ptr(), N, P.data_ptr(), N,
                                               flags | rt._lib.RTK_SCORE_KERNEL_WS, sp), "ws")
    return P


def _reference(rt, core, R, S, O, h, r, t, flt, mode, want_bce=False):
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, h.numel(), O, _flags(rt, mode))
    ids = torch.arange(h.numel()).cuda() if flt is not None else None
    return rt.filtered_ranks(P, t, flt, ids, want_bce=want_bce)


def _problem(n_ent, c, B, seed, gain=1.0, dtype=torch.float32, shared=False, n_rel=7):
    rank = (6, c, c)
    core, R, S, O = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, rank, seed, shared=shared)]
    O = O * gain
    if shared:
        S = O
    h, r = [torch.from_numpy(x).cuda() for x in gen.make_queries(n_ent, n_rel, B, seed)]
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.integers(0, n_ent, B)).cuda()
    if dtype != torch.float32:
        core, R, S, O = core.to(dtype), R.to(dtype), S.to(dtype), O.to(dtype)
        if shared:
            S = O
    return core, R, S, O, h, r, t


def _filter(n_ent, t, seed):
    """Per query: empty lists, lists holding the target, lists with out-of-range and repeated-free entries."""
    rng = np.random.default_rng(seed + 1)
    tt = t.cpu().numpy()
    lists, slots = [], []
    for d in range(len(tt)):
        k = d % 4
        if k == 0:
            slots.append(-1)
            continue
        m = int(rng.integers(0, 40)) if k != 3 else 0
        objs = rng.choice(n_ent, size=min(m, n_ent), replace=False).tolist()
        if k == 1:
            objs.append(int(tt[d]))                 # the target itself is in the list
        if k == 2 and d % 8 == 2:
            objs.append(n_ent + 5)                  # skipped, as by filtered_rank_kernel
        slots.append(len(lists))
        lists.append(objs)
    if not lists:
        lists.append([])
    return Flt(lists, slots)


SHAPES_F32 = [
    # (N, c, B, gain)
    (40943, 200, 512, 1.0),       # WN18RR shape
    (40943, 200, 500, 40.0),      # ragged last query tile; saturated: many p == 1.0 exactly
    (20000, 200, 64, 1.0),
    (36000, 64, 40, 40.0),
    (2000, 200, 64, 1.0),
    (333, 36, 70, 40.0),          # KS = 3, N % 32 != 0
    (100, 4, 5, 1.0),             # KS = 1
    (20, 8, 33, 40.0),            # fewer entities than one group
    (167, 208, 96, 1.0),          # KS = 13
    (100000, 64, 40, 1.0),
]


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B,gain", SHAPES_F32)
def test_f32_ranks_equal_ws_scores(rt, N, c, B, gain, mode):
    core, R, S, O, h, r, t = _problem(N, c, B, N + c, gain)
    flt = _filter(N, t, N)
    for f in (None, flt):
        ref = _reference(rt, core, R, S, O, h, r, t, f, mode)
        got = rt.rank_1vN(core, R, S, O, h, r, t, flt=f, sigmoid_mode=mode)
        assert got.dtype == torch.int32 and got.shape == (B,)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    ref_r, ref_b = _reference(rt, core, R, S, O, h, r, t, flt, mode, want_bce=True)
    got_r, got_b = rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, want_bce=True, sigmoid_mode=mode)
    np.testing.assert_array_equal(got_r.cpu().numpy(), ref_r.cpu().numpy())
    assert got_b.dtype == torch.float64
    torch.testing.assert_close(got_b, ref_b, rtol=1e-6, atol=1e-6)
    if gain > 1.0 and mode == "exact":
        _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
        P = _stored_scores(rt, qp, B, O, _flags(rt, mode))
        assert (P == 1.0).float().mean().item() > 0.05          # the tie-heavy case is really tie heavy


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B", [(14541, 200, 2048), (3000, 512, 96), (777, 18, 70), (500, 72, 33)])
def test_bf16_ranks_equal_bf16_scores(rt, N, c, B, mode):
    core, R, S, O, h, r, t = _problem(N, c, B, c, 8.0, dtype=torch.bfloat16, shared=True)
    flt = _filter(N, t, c)
    for f in (None, flt):
        ref = _reference(rt, core, R, S, O, h, r, t, f, mode)
        got = rt.rank_1vN(core, R, O, O, h, r, t, flt=f, sigmoid_mode=mode)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())
    if (N, c, B) == (14541, 200, 2048):         # the model path (score_1vN) gives the same scores
        P = rt.score_1vN(core, R, O, O, h, r, sigmoid_mode=mode)
        ref = rt.filtered_ranks(P, t, flt, torch.arange(B).cuda())
        got = rt.rank_1vN(core, R, O, O, h, r, t, flt=flt, sigmoid_mode=mode)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())


def test_geometry_and_determinism(rt):
    N, c, B = 5000, 200, 300
    core, R, S, O, h, r, t = _problem(N, c, B, 5, 40.0)
    flt = _filter(N, t, 5)
    full, bce = rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, want_bce=True)
    again, bce2 = rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, want_bce=True)
    assert torch.equal(full, again) and torch.equal(bce, bce2)
    slots = flt.slot_of_item
    parts = []
    for lo, hi in ((0, 117), (117, B)):
        flt.slot_of_item = slots[lo:hi]
        parts.append(rt.rank_1vN(core, R, S, O, h[lo:hi], r[lo:hi], t[lo:hi], flt=flt))
    assert torch.equal(torch.cat(parts), full)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(B)).cuda()
    flt.slot_of_item = slots[perm]
    assert torch.equal(rt.rank_1vN(core, R, S, O, h[perm], r[perm], t[perm], flt=flt), full[perm])


def test_errors_and_edges(rt):
    N, c, B = 300, 32, 40
    core, R, S, O, h, r, t = _problem(N, c, B, 9)
    bad = t.clone()
    bad[3] = N
    with rt.index_check("deferred"):
        rt.rank_1vN(core, R, S, O, h, r, bad)
        with pytest.raises(IndexError, match="object_idx"):
            rt.check_device_errors()
        hb = h.clone()
        hb[0] = N + 2
        rt.rank_1vN(core, R, S, O, hb, r, t)
        with pytest.raises(IndexError):
            rt.check_device_errors()
        rt.check_device_errors()                     # the word was cleared
    with pytest.raises(IndexError):                  # strict (default): raised by the call itself
        rt.rank_1vN(core, R, S, O, h, r, bad)
    e = torch.zeros(0, dtype=torch.int64).cuda()
    out = rt.rank_1vN(core, R, S, O, e, e, e)
    assert out.shape == (0,) and out.dtype == torch.int32
    rk, bce = rt.rank_1vN(core, R, S, O, e, e, e, want_bce=True)
    assert rk.shape == (0,) and bce.shape == (0,)
    # N = 1: every rank is 1
    core1, R1, S1, O1, h1, r1, _ = _problem(1, c, 7, 3)
    t1 = torch.zeros(7, dtype=torch.int64).cuda()
    assert torch.equal(rt.rank_1vN(core1, R1, S1, O1, h1, r1, t1).cpu(), torch.ones(7, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="above 208"):
        core2, R2, S2, O2, h2, r2, t2 = _problem(50, 224, 4, 1)
        rt.rank_1vN(core2, R2, S2, O2, h2, r2, t2)


@pytest.mark.parametrize("sym", [False, True])
def test_model_rank_equals_ops(rt, sym):
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
    got, bce = model.rank_objects(h, r, t, flt=flt, want_bce=True)
    ref, rbce = rt.rank_1vN(model.core, model.R.weight, S, O, h, r, t, flt=flt, want_bce=True)
    assert torch.equal(got, ref) and torch.equal(bce, rbce)


@pytest.mark.parametrize("variant", ["planted", "planted_sat", "spread"])
def test_wn18rr(rt, golden_meta, variant):
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    n_ent, n_rel, rank, seed = len(data.entities), len(data.relations), (10, 200, 200), 322
    test = KG_dataset(data, data.test_data, test_set=True)
    if variant.startswith("planted"):
        train = KG_dataset(data, data.train_data, label_smoothing=0.1)
        valid = KG_dataset(data, data.valid_data, test_set=True)
        planted = np.concatenate([np.asarray(train.data_index, dtype=np.int64), valid.features[::2], test.features[::2]])
        params = gen.make_planted_params(planted, n_ent, n_rel, rank, seed, gain=8.0 if variant == "planted" else 40.0)
    else:
        params = gen.make_params(n_ent, n_rel, rank, seed)
    core, R, S, O = [torch.from_numpy(x).cuda() for x in params]
    flt = rt.DeviceFilter(test, "cuda")
    n = len(test)
    all_ranks = []
    for lo in range(0, n, 512):
        ids = torch.arange(lo, min(lo + 512, n)).cuda()
        f = flt.features[ids]
        got, bce = rt.rank_1vN(core, R, S, O, f[:, 0], f[:, 1], f[:, 2], flt=flt, want_bce=True)
        if lo == 0:
            _, qp = rt.query_vectors(core, R, S, f[:, 0], f[:, 1], packed=True)
            flags = rt._lib.RTK_SCORE_SIGMOID | (rt._lib.RTK_SCORE_SIGMOID_FAST if rt.ops.DEFAULT_SIGMOID == "fast" else 0)
            P = _stored_scores(rt, qp, ids.numel(), O, flags)
            ref = orc.filter_and_rank_stable(P.cpu(), test.dense_targets(np.arange(ids.numel())), f[:, 2].cpu())
            np.testing.assert_array_equal(got.cpu().numpy(), ref.numpy())
            # BCE: within 1e-6 of the float64 sum over the same probabilities; filtered_ranks' own sums carry fp32
            # partials of N / 256 terms each, so the two fp32-partial results agree to ~1e-6 (measured 1.3e-6 at most)
            y = torch.as_tensor(test.dense_targets(np.arange(ids.numel()))).cuda().double()
            P64 = P.double()
            ref64 = -(y * P64.log().clamp(min=-100) + (1 - y) * (1 - P64).log().clamp(min=-100)).sum(1)
            torch.testing.assert_close(bce, ref64, rtol=1e-6, atol=1e-6)
            _, ref_bce = rt.filtered_ranks(P, f[:, 2], flt, ids, want_bce=True)
            torch.testing.assert_close(bce, ref_bce, rtol=2e-6, atol=1e-6)
            print(f"BCE vs float64: {((bce - ref64).abs() / ref64.abs()).max().item():.2e}, filtered_ranks vs float64: "
                  f"{((ref_bce - ref64).abs() / ref64.abs()).max().item():.2e} (max relative)")
        all_ranks.append(got)
    ranks = torch.cat(all_ranks).double()
    mrr = (1.0 / ranks).mean().item()
    case = golden_meta["cases"][f"rank_{variant}_test"]
    print(f"\n{variant}: rank_1vN MRR {mrr:.6f} (reference {case['mrr']:.6f})")
    if variant != "planted_sat":
        assert abs(mrr - case["mrr"]) <= 1e-3


def test_one_million_entities_bf16(rt):
    """1 M entities, c = 512, bf16, B 8192: ranks equal a blockwise reference built from existing entry points, and
    the call allocates far less than the 32.8 GB score matrix."""
    from r_tucker_amd.evaluation import rank_counts_block, target_scores_block
    N, c, B, n_rel = 1_000_000, 512, 8192, 11
    g = torch.Generator(device="cuda").manual_seed(0)
    core = (torch.randn((4, c, c), device="cuda", generator=g) * (3.0 / np.sqrt(4 * c * c))).to(torch.bfloat16)
    R = torch.randn((n_rel, 4), device="cuda", generator=g).to(torch.bfloat16)
    E = (torch.randn((N, c), device="cuda", generator=g) / np.sqrt(c) * 4).to(torch.bfloat16)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    t = torch.randint(0, N, (B,), device="cuda", generator=g)
    flags = _flags(rt, "fast")
    _, qp = rt.query_vectors(core, R, E, h, r, packed=True)
    # the blockwise reference needs block-width-independent bf16 bits: one block against a full-width score
    nb = 1 << 16
    Ns = 3 * nb
    full = _stored_scores(rt, qp[:rt._lib.load().rtk_packed_query_bytes(1, 64, c)], 64, E[:Ns], flags)
    blk = _stored_scores(rt, qp[:rt._lib.load().rtk_packed_query_bytes(1, 64, c)], 64, E[nb:2 * nb], flags)
    assert torch.equal(full[:, nb:2 * nb], blk)
    del full, blk
    pts = []
    for lo in range(0, N, nb):
        P = _stored_scores(rt, qp, B, E[lo:lo + nb], flags)
        pts.append(target_scores_block(P, t, lo))
    pt = torch.stack(pts).max(dim=0).values
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    for lo in range(0, N, nb):
        P = _stored_scores(rt, qp, B, E[lo:lo + nb], flags)
        counts += rank_counts_block(P, t, lo, pt)
    del P
    ref = counts + 1
    tables = rt.relation_tables(core, R)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    got = rt.rank_1vN(core, R, E, E, h, r, t, sigmoid_mode="fast", tables=tables)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"\n1M bf16: peak growth {grown / 2**20:.1f} MiB")
    assert grown < 256 << 20
    np.testing.assert_array_equal(got.cpu().numpy(), ref.cpu().numpy())


def test_trained_checkpoint(rt):
    """The committed trained WN18RR model (tests/golden/wn18rr_trained_q8.npz), test split in batches of 512: ranks equal
    filtered_ranks over the ws-scored matrix batch by batch, and MRR / hits@1/3/10 are within 1e-3 of evaluate()'s (the
    difference comes only from the column-group kernel's fifth-group bits)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from configs.base_config import wn18rr_readme_config
    from r_tucker_amd.data import Data, KG_dataset
    from pack_checkpoint_q8 import dequantise
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
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
    model.cuda().eval()
    test = KG_dataset(data, data.test_data, test_set=True)
    flt = rt.DeviceFilter(test, "cuda")
    dev_metrics, _ = rt.evaluate(model, test, batch_size=512, flt=flt)
    core, R, S, O = model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data
    flags = rt._lib.RTK_SCORE_SIGMOID | (rt._lib.RTK_SCORE_SIGMOID_FAST if rt.ops.DEFAULT_SIGMOID == "fast" else 0)
    n = len(test)
    ranks = []
    tables = rt.relation_tables(core, R)            # the stage 1 that rank_objects runs in eval mode (cached tables)
    with torch.no_grad():
        for lo in range(0, n, 512):
            ids = torch.arange(lo, min(lo + 512, n), device="cuda")
            f = flt.features[ids]
            got = model.rank_objects(f[:, 0], f[:, 1], f[:, 2], flt=flt)
            _, qp = rt.query_vectors(core, R, S, f[:, 0], f[:, 1], tables=tables, packed=True)
            ref = rt.filtered_ranks(_stored_scores(rt, qp, ids.numel(), O, flags), f[:, 2], flt, ids)
            assert torch.equal(got, ref), lo
            ranks.append(got)
    sums = rt.metrics_from_ranks(torch.cat(ranks))
    keys = ("mrr", "hits@1", "hits@3", "hits@10")
    mine = {k: float(sums[k]) / n for k in keys}
    print("\nrank_1vN - evaluate(): " + ", ".join(f"{k} {mine[k] - float(dev_metrics[k]):+.2e}" for k in keys))
    for k in keys:
        assert abs(mine[k] - float(dev_metrics[k])) <= 1e-3, (k, mine[k], dev_metrics[k])
