"""GPU tests of filtered ranking on entity blocks without the score block (ops.rank_targets_block,
ops.rank_counts_block_1vN, ShardedEntityScorer.rank_1vN; rtk_score_rank_targets_* / rtk_score_rank_counts_*,
csrc/rtk_score_rank.hip).

Ranks are integers and a probability's bits depend only on its query row, its entity row and c, so every check on
counts is exact: for each way of cutting the entity range into blocks, 1 + the sum of the blocks' counts must EQUAL
ops.rank_1vN on the whole range, and the target score on the owning block must have the bits of the stored score
kernel's column (fp32: the ws kernel, bf16: rtk_score_packed_bf16).  BCE shares are float sums in another order:
rtol 2e-6, atol 1e-6 (the tolerance between the project's two existing BCE paths), and bit-identical on repetition."""
import os

import numpy as np
import pytest
import torch

import gen

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
    """Per query: no list, lists that hold the target, a repeated object, ids outside [0, n_ent), long lists (more than
    one filter wave's 32 entries, more than all eight waves' 256), an empty list."""
    rng = np.random.default_rng(seed + 1)
    tt = t.cpu().numpy()
    lists, slots = [], []
    for d in range(len(tt)):
        k = d % 4
        if k == 0:
            slots.append(-1)
            continue
        m = int(rng.integers(0, 40)) if k != 3 else 0
        if d % 16 == 5:
            m = 300
        objs = rng.choice(n_ent, size=min(m, n_ent), replace=False).tolist()
        if k == 1:
            objs.append(int(tt[d]))                 # the target itself is in the list
        if k == 2 and objs:
            objs.append(objs[0])                    # an object listed twice (rank_1vN sees the same list)
        if k == 2 and d % 8 == 2:
            objs.append(n_ent + 5)                  # outside every block
        slots.append(len(lists))
        lists.append(objs)
    if not lists:
        lists.append([])
    return Flt(lists, slots)


def _cuts(N):
    """One block; two unequal blocks whose boundary is not a multiple of 32; eight blocks of ceil(N / 8), the last
    one short (or missing when N is small)."""
    cuts = [[(0, N)]]
    if N >= 2:
        b = max(1, min(N - 1, (N * 3) // 8 | 1))
        if b % 32 == 0:
            b += 1
        cuts.append([(0, b), (b, N)])
    n8 = -(-N // 8)
    cuts.append([(lo, min(lo + n8, N)) for lo in range(0, N, n8)])
    return cuts


def _flags(rt, mode):
    L = rt._lib
    return L.RTK_SCORE_SIGMOID | (L.RTK_SCORE_SIGMOID_FAST if mode == "fast" else 0)


def _stored_scores(rt, qp, B, O, flags):
    """(B, N) fp32 probabilities of the stored score kernel the header names as reference: fp32 operands through the ws
    kernel, bf16 through rtk_score_packed_bf16."""
    lib = rt._lib.load()
    O = O.contiguous()
    N, c = O.shape
    P = torch.empty((B, N), dtype=torch.float32, device=O.device)
    sp = torch.cuda.current_stream().cuda_stream
    if O.dtype == torch.bfloat16:
        rt._lib.check(lib.rtk_score_packed_bf16(qp.data_ptr(), B, c, O.data_ptr(), N, P.data_ptr(), N, flags, sp), "bf16")
    else:
        rt._lib.check(lib.rtk_score_packed_f32(qp.data_ptr(), B, c, O.data_ptr(), N, P.data_ptr(), N,
                                               flags | rt._lib.RTK_SCORE_KERNEL_WS, sp), "ws")
    return P


def _blocks(rt, qp, B, O, cut, t, flt, mode, want_bce=False, check_pt=None):
    """pt (maximum over the blocks), summed counts and summed BCE shares of one cut."""
    N = O.shape[0]
    slots = flt.slot_of_item if flt is not None else None
    pts = [rt.rank_targets_block(qp, B, O[lo:hi], lo, N, t, sigmoid_mode=mode) for lo, hi in cut]
    for (lo, hi), p in zip(cut, pts):
        own = (t >= lo) & (t < hi)
        assert torch.isneginf(p[~own]).all()                     # -inf on every block that does not own the object
        if check_pt is not None:                                 # bit for bit the stored kernel's target column
            assert torch.equal(p[own], check_pt[own])
    pt = pts[0]
    for p in pts[1:]:
        pt = torch.maximum(pt, p)
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    bce = torch.zeros(B, dtype=torch.float64, device="cuda")
    for lo, hi in cut:
        res = rt.rank_counts_block_1vN(qp, B, O[lo:hi], lo, N, pt, t, flt=flt, slots=slots, want_bce=want_bce,
                                       sigmoid_mode=mode)
        if want_bce:
            assert res[0].dtype == torch.int32 and res[1].dtype == torch.float64
            counts += res[0]
            bce += res[1]
        else:
            assert res.dtype == torch.int32 and res.shape == (B,)
            counts += res
    return pt, counts, bce


def _check_problem(rt, core, R, S, O, h, r, t, flt, mode, bce=True):
    B, N = h.numel(), O.shape[0]
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, B, O, _flags(rt, mode))
    col = P[torch.arange(B, device="cuda"), t]
    del P
    for f in (None, flt):
        want = rt.rank_1vN(core, R, S, O, h, r, t, flt=f, sigmoid_mode=mode)
        for cut in _cuts(N):
            pt, counts, _ = _blocks(rt, qp, B, O, cut, t, f, mode, check_pt=col)
            assert torch.equal(pt, col)
            np.testing.assert_array_equal((counts + 1).cpu().numpy(), want.cpu().numpy(), err_msg=f"cut {cut[:3]}")
    if bce:
        want, want_bce = rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, want_bce=True, sigmoid_mode=mode)
        for cut in _cuts(N):
            _, counts, got = _blocks(rt, qp, B, O, cut, t, flt, mode, want_bce=True)
            _, counts2, again = _blocks(rt, qp, B, O, cut, t, flt, mode, want_bce=True)
            np.testing.assert_array_equal((counts + 1).cpu().numpy(), want.cpu().numpy())
            assert torch.equal(got, again) and torch.equal(counts, counts2)       # repeated calls: the same bits
            d = (got - want_bce).abs()
            print(f"BCE shares vs rank_1vN, {len(cut)} block(s): max abs {d.max().item():.3e}, "
                  f"max rel {(d / want_bce.abs().clamp(min=1e-30)).max().item():.3e}")
            torch.testing.assert_close(got, want_bce, rtol=2e-6, atol=1e-6)


SHAPES_F32 = [
    # (N, c, B, gain): the list of tests/test_gpu_rank.py
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
def test_f32_blocks_equal_rank_1vN(rt, N, c, B, gain, mode):
    core, R, S, O, h, r, t = _problem(N, c, B, N + c, gain)
    _check_problem(rt, core, R, S, O, h, r, t, _filter(N, t, N), mode)
    if gain > 1.0 and mode == "exact":
        _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
        P = _stored_scores(rt, qp, B, O, _flags(rt, mode))
        assert (P == 1.0).float().mean().item() > 0.05          # the tie-heavy case is really tie heavy


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("N,c,B", [(14541, 200, 2048), (3000, 512, 96), (777, 18, 70), (500, 72, 33)])
def test_bf16_blocks_equal_rank_1vN(rt, N, c, B, mode):
    core, R, S, O, h, r, t = _problem(N, c, B, c, 8.0, dtype=torch.bfloat16, shared=True)
    _check_problem(rt, core, R, O, O, h, r, t, _filter(N, t, c), mode)


@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_zero_target_score_ties_with_filtered_objects(rt, mode):
    """Packed planes built from chosen logits (bf16, O = unit rows): rows whose target probability is exactly 0 tie with
    the filtered objects (which count as 0) and with other zeros, rows of exact ones and repeated values -- the
    pattern of tests/golden/ties.npz, widened to 70 entities so that the blocks cut through the ties."""
    lib = rt._lib.load()
    z = np.load(os.path.join(ROOT, "tests", "golden", "ties.npz"))
    Pz = z["P"].astype(np.float64).clip(1e-9, 1 - 1e-9)
    base = np.where(z["P"] >= 1.0, 40.0, np.where(z["P"] <= 0.0, -200.0, np.log(Pz / (1 - Pz))))
    N, c, B = 70, 80, 36
    rng = np.random.default_rng(3)
    logits = np.tile(base, (B // 3, 12))[:, :N].astype(np.float32)
    logits[:, 40:] = rng.choice(np.asarray([-200.0, -1.0, 0.0, 40.0], np.float32), size=(B, N - 40))
    t = torch.from_numpy(rng.integers(0, N, B)).cuda()
    logits[np.arange(B)[::2], t.cpu().numpy()[::2]] = -200.0          # every other target scores exactly 0
    v = torch.zeros((B, c), dtype=torch.float32)
    v[:, :N] = torch.from_numpy(logits)
    O = torch.zeros((N, c), dtype=torch.bfloat16)
    O[torch.arange(N), torch.arange(N)] = 1.0
    v, O = v.cuda(), O.cuda()
    qp = rt.pack_query_vectors(v, torch.bfloat16)
    flt = _filter(N, t, 3)
    flags = _flags(rt, mode)
    P = _stored_scores(rt, qp, B, O, flags)
    col = P[torch.arange(B, device="cuda"), t]
    assert (col == 0.0).sum().item() >= B // 2
    sp = torch.cuda.current_stream().cuda_stream
    for f in (None, flt):
        want = torch.empty(B, dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.rtk_score_rank_workspace_bytes(1, B, N, c) + 256, dtype=torch.uint8, device="cuda")
        ws[:256].zero_()
        rt._lib.check(lib.rtk_score_rank_bf16(qp.data_ptr(), B, c, O.data_ptr(), N, t.data_ptr(),
                                              f.slot_of_item.data_ptr() if f else None,
                                              f.pair_ptr.data_ptr() if f else None, f.pair_obj.data_ptr() if f else None,
                                              flags, want.data_ptr(), None, ws.data_ptr(), ws.numel(), sp), "rank")
        for cut in _cuts(N):
            pt, counts, _ = _blocks(rt, qp, B, O, cut, t, f, mode, check_pt=col)
            np.testing.assert_array_equal((counts + 1).cpu().numpy(), want.cpu().numpy())


@pytest.mark.parametrize("variant", ["planted", "planted_sat", "spread"])
def test_wn18rr_batches(rt, variant):
    """The WN18RR fixture problems (the parameters behind tests/golden/wn18rr_rank.npz), test split, batch by batch,
    in 1 and in 3 blocks, with the dataset's own filter lists."""
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
    _wn18rr_batches(rt, core, R, S, O, rt.DeviceFilter(test, "cuda"), len(test), bce_first=True)


def _wn18rr_batches(rt, core, R, S, O, flt, n, bce_first=False):
    N = O.shape[0]
    b1, b2 = N // 3 + 5, 2 * N // 3 + 11
    for lo in range(0, n, 512):
        f = flt.features[lo:min(lo + 512, n)]
        h, r, t = f[:, 0].contiguous(), f[:, 1].contiguous(), f[:, 2].contiguous()
        B = h.numel()
        slots = flt.slots_of(h, r)
        bce = bce_first and lo == 0
        res = rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, want_bce=bce)
        want, want_bce = res if bce else (res, None)
        _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
        for cut in ([(0, N)], [(0, b1), (b1, b2), (b2, N)]):
            pt = None
            for a, b in cut:
                p = rt.rank_targets_block(qp, B, O[a:b], a, N, t)
                pt = p if pt is None else torch.maximum(pt, p)
            counts = torch.zeros(B, dtype=torch.int32, device="cuda")
            shares = torch.zeros(B, dtype=torch.float64, device="cuda")
            for a, b in cut:
                res = rt.rank_counts_block_1vN(qp, B, O[a:b], a, N, pt, t, flt=flt, slots=slots, want_bce=bce)
                counts += res[0] if bce else res
                if bce:
                    shares += res[1]
            assert torch.equal(counts + 1, want), (lo, len(cut))
            if bce:
                torch.testing.assert_close(shares, want_bce, rtol=2e-6, atol=1e-6)


def test_trained_checkpoint_batches(rt):
    """The committed trained WN18RR model (tests/golden/wn18rr_trained_q8.npz), test split in batches of 512, in 1 and
    in 3 blocks: equal to rank_1vN batch by batch."""
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
    core, R, S, O = model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data.contiguous()
    _wn18rr_batches(rt, core, R, S, O, rt.DeviceFilter(test, "cuda"), len(test))


def test_one_million_entities_bf16_in_8_blocks(rt):
    """1 M entities, c = 512, bf16, B 8192 in eight blocks of 125 000 against rank_1vN on the whole range; the eight
    block calls together allocate far less than one block's 4.1 GB of scores."""
    N, c, B, n_rel = 1_000_000, 512, 8192, 11
    g = torch.Generator(device="cuda").manual_seed(0)
    core = (torch.randn((4, c, c), device="cuda", generator=g) * (3.0 / np.sqrt(4 * c * c))).to(torch.bfloat16)
    R = torch.randn((n_rel, 4), device="cuda", generator=g).to(torch.bfloat16)
    E = (torch.randn((N, c), device="cuda", generator=g) / np.sqrt(c) * 4).to(torch.bfloat16)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    t = torch.randint(0, N, (B,), device="cuda", generator=g)
    tables = rt.relation_tables(core, R)
    want = rt.rank_1vN(core, R, E, E, h, r, t, sigmoid_mode="fast", tables=tables)
    _, qp = rt.query_vectors(core, R, E, h, r, tables=tables, packed=True)
    n8 = N // 8
    rt.rank_targets_block(qp, B, E[:n8], 0, N, t, sigmoid_mode="fast")          # (the workspace of the stream exists)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    pt = None
    for lo in range(0, N, n8):
        p = rt.rank_targets_block(qp, B, E[lo:lo + n8], lo, N, t, sigmoid_mode="fast")
        pt = p if pt is None else torch.maximum(pt, p)
    counts = torch.zeros(B, dtype=torch.int32, device="cuda")
    for lo in range(0, N, n8):
        counts += rt.rank_counts_block_1vN(qp, B, E[lo:lo + n8], lo, N, pt, t, sigmoid_mode="fast")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f"\n1M bf16 in 8 blocks: peak growth {grown / 2**20:.1f} MiB")
    assert grown < 256 << 20
    np.testing.assert_array_equal((counts + 1).cpu().numpy(), want.cpu().numpy())


def test_sharded_scorer_world1_and_errors(rt):
    N, c, B = 3000, 32, 70
    core, R, S, O, h, r, t = _problem(N, c, B, 9)
    flt = _filter(N, t, 9)
    sc = rt.ShardedEntityScorer(N)
    O_loc = sc.local_block(O)
    want, want_bce = rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, want_bce=True)
    got, bce = sc.rank_1vN(core, R, S, O_loc, h, r, t, flt=flt, want_bce=True)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    torch.testing.assert_close(bce, want_bce, rtol=2e-6, atol=1e-6)
    assert torch.equal(sc.rank_1vN(core, R, S, O_loc, h, r, t), rt.rank_1vN(core, R, S, O, h, r, t))
    tables = rt.relation_tables(core, R)
    assert torch.equal(sc.rank_1vN(core, R, S, O_loc, h, r, t, flt=flt, tables=tables, sigmoid_mode="exact"),
                       rt.rank_1vN(core, R, S, O, h, r, t, flt=flt, tables=tables, sigmoid_mode="exact"))
    bad = t.clone()
    bad[3] = N
    with pytest.raises(IndexError, match="object_idx"):          # strict (default): raised by the call itself
        sc.rank_1vN(core, R, S, O_loc, h, r, bad)
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    with rt.index_check("deferred"):
        rt.rank_targets_block(qp, B, O[:100], 0, N, bad)
        with pytest.raises(IndexError, match="object_idx"):
            rt.check_device_errors()
        rt.check_device_errors()                                 # the word was cleared
    e = torch.zeros(0, dtype=torch.int64).cuda()
    _, qp0 = rt.query_vectors(core, R, S, e, e, packed=True)
    assert rt.rank_targets_block(qp0, 0, O, 0, N, e).shape == (0,)
    cnt, b0 = rt.rank_counts_block_1vN(qp0, 0, O, 0, N, torch.zeros(0, device="cuda"), e, want_bce=True)
    assert cnt.shape == (0,) and cnt.dtype == torch.int32 and b0.shape == (0,)
    with pytest.raises(RuntimeError, match="above 208"):
        core2, R2, S2, O2, h2, r2, t2 = _problem(50, 224, 4, 1)
        _, qp2 = rt.query_vectors(core2, R2, S2, h2, r2, packed=True)
        rt.rank_targets_block(qp2, 4, O2, 0, 50, t2)
