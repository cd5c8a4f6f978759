"""The 1-vs-all BCE loss without the (B, N) score matrix (rtk_bce_stream_* behind bce_loss_1vN(matrix_free=True)):
against the oracle, against float64 on the sweep's own probabilities (saturation), against the matrix form on a
training-sized batch, peak memory, determinism, refusals, graph capture and a short optimizer run."""
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
    assert torch.cuda.is_available()
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


class _Pairs:
    """The attributes DeviceFilter reads from a KG_dataset, for a synthetic (pair -> objects) table."""
    def __init__(self, pairs, lists, n_ent, eps):
        self._pair_slot = {p: i for i, p in enumerate(pairs)}
        self._ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        self._obj = np.asarray([x for l in lists for x in l], dtype=np.int64)
        self.features = np.asarray(pairs, dtype=np.int64)
        self.n_ent, self.label_smoothing = n_ent, eps

    def dense(self, ids, dtype=torch.float32):
        t = torch.zeros((len(ids), self.n_ent), dtype=dtype)
        for row, i in enumerate(ids):
            t[row, self._obj[self._ptr[i]:self._ptr[i + 1]]] = 1
        return (1 - self.label_smoothing) * t + self.label_smoothing / self.n_ent


def _batch(n_ent, n_rel, B, seed, eps, max_len=9, empty=False, n_pairs=200):
    """A synthetic pair table and a batch of B of its items (with repeats when there are fewer pairs than B)."""
    rng = np.random.default_rng(seed)
    n_pairs = min(n_pairs, n_ent)
    pairs = [(int(s), int(r)) for s, r in zip(rng.permutation(n_ent)[:n_pairs], rng.integers(0, n_rel, n_pairs))]
    lists = [rng.integers(0, n_ent, rng.integers(1, max_len)).tolist() for _ in pairs]
    lists[min(3, n_pairs - 1)] = lists[min(3, n_pairs - 1)] * 2          # repeated triples: every object counts once
    ids = rng.permutation(n_pairs)[:B] if B <= n_pairs else rng.integers(0, n_pairs, B)
    if empty:
        lists[int(ids[0])] = []                                          # a query without known objects
    return _Pairs(pairs, lists, n_ent, eps), np.asarray(ids, dtype=np.int64)


def _flags(rt, mode):
    return rt._lib.RTK_SCORE_SIGMOID | (rt._lib.RTK_SCORE_SIGMOID_FAST if mode == "fast" else 0)


def _abi(rt, core, R, S, O, h, r, slot, flt, eps, mode, max_pos, scale=1.0, want_dv=True):
    """rows, dv, gO through the two ABI calls on fresh buffers."""
    lib = rt._lib.load()
    v, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    B, (N, c) = h.numel(), O.shape
    ws = torch.zeros(lib.rtk_bce_stream_workspace_bytes(B, N, c, max_pos), dtype=torch.uint8, device="cuda")
    rows = torch.empty(B, dtype=torch.float64, device="cuda")
    dv = torch.empty((B, c), dtype=torch.float32, device="cuda")
    gO = torch.empty((N, c), dtype=torch.float32, device="cuda")
    sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    rt._lib.check(lib.rtk_bce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), N, *csr, eps, _flags(rt, mode),
                                              rows.data_ptr(), dv.data_ptr() if want_dv else None, ws.data_ptr(), ws.numel(),
                                              sp), "rows")
    rt._lib.check(lib.rtk_bce_stream_grad_o_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), N, *csr, max_pos, eps,
                                                _flags(rt, mode), sc.data_ptr(), gO.data_ptr(), ws.data_ptr(), ws.numel(),
                                                sp), "grad_o")
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0
    return rows, dv, gO, v, qp


def _check_oracle(rt, n_ent, rank, B, mode, eps, smode, core_scale, empty, seed=41):
    n_rel = 7
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, seed, shared=(mode == "sym"))
    core = (core * core_scale).astype(np.float32)
    ds, ids = _batch(n_ent, n_rel, B, seed, eps, empty=empty)
    h = torch.from_numpy(ds.features[ids, 0].copy())
    r = torch.from_numpy(ds.features[ids, 1].copy())
    tc, tR, tS, tO = [torch.from_numpy(x) for x in (core, R, S, O)]
    if core_scale != 1.0:        # the comparison with an implementation that knows no saturation needs unsaturated scores
        z = orc.logits_ref(tc.double(), tR.double(), tS.double(), (tS if mode == "sym" else tO).double(), h, r)
        assert z.abs().max().item() < 12.0
    ref = orc.bce_loss_grads_ref(tc, tR, tS, tO, h, r, ds.dense(ids), shared=(mode == "sym"))

    flt = rt.DeviceFilter(ds, "cuda")
    dc, dR, dS = [x.clone().cuda().requires_grad_(True) for x in (tc, tR, tS)]
    dO = dS if mode == "sym" else tO.clone().cuda().requires_grad_(True)
    loss = rt.bce_loss_1vN(dc, dR, dS, dO, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(), label_smoothing=eps,
                           matrix_free=True, sigmoid_mode=smode)
    print(f"loss {loss.item():.9g} ref {ref[0].item():.9g}")
    assert abs(loss.item() - ref[0].item()) <= 2e-6 * max(1.0, abs(ref[0].item()))
    (loss * 3.0).backward()                                # a non-unit upstream gradient
    got = [dc.grad, dR.grad, dS.grad] + ([] if mode == "sym" else [dO.grad])
    for g, e in zip(got, ref[1:]):
        e = 3.0 * e
        assert g.shape == e.shape
        err = (g.cpu() - e).abs().max().item()
        print(f"grad {tuple(e.shape)}: err {err:.3e} of max {e.abs().max().item():.3e}")
        assert err <= 2e-4 * e.abs().max().item() + 1e-9


@pytest.mark.parametrize("mode", ["asym", "sym"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_and_gradients_against_oracle(rt, mode, eps):
    """The cases and bounds of test_gpu_loss.py::test_loss_and_gradients_against_oracle through matrix_free=True."""
    _check_oracle(rt, 3001, (5, 32, 32), 48, mode, eps, None, 1.0, False)


@pytest.mark.parametrize("smode", ["fast", "exact"])
@pytest.mark.parametrize("c,B,n_ent", [(4, 1, 31), (100, 33, 3003), (200, 70, 3003), (208, 70, 31), (208, 33, 3003),
                                      (4, 70, 3003), (200, 1, 31)])
def test_edges_of_the_range_against_oracle(rt, c, B, n_ent, smode):
    """The same bounds at the edges of the covered range, with a query whose CSR list is empty; the core is scaled by 0.4
    so that no score saturates (asserted from the oracle's float64 logits)."""
    _check_oracle(rt, n_ent, (5, c, c), B, "asym", 0.1, smode, 0.4, True)


@pytest.mark.parametrize("smode", ["fast", "exact"])
@pytest.mark.parametrize("c", [64, 208])
def test_saturated_scores_against_float64_on_the_sweeps_probabilities(rt, c, smode):
    """Logits scaled until ws-kernel scores are exactly 1.0f / 0.0f: loss rows (logs clamped at -100), dv and gO from
    the ABI calls against float64 formed on the host from the stored ws scores -- zero logit gradient where saturated."""
    n_ent, n_rel, B, eps = 3003, 7, 70, 0.1
    core, R, S, O = gen.make_params(n_ent, n_rel, (3, c, c), 43)
    core = core * 40.0
    ds, ids = _batch(n_ent, n_rel, B, 43, eps, max_len=12, n_pairs=120)
    flt = rt.DeviceFilter(ds, "cuda")
    core, R, S, O = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (core, R, S, O)]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    slot = flt.slot_of_item[torch.from_numpy(ids).cuda()].contiguous()
    max_pos = B * flt.max_list
    lib = rt._lib.load()
    for e in (eps, 0.0):
        rows, dv, gO, v, qp = _abi(rt, core, R, S, O, h, r, slot, flt, e, smode, max_pos)
        P = torch.empty((B, n_ent), dtype=torch.float32, device="cuda")
        rt._lib.check(lib.rtk_score_packed_f32(qp.data_ptr(), B, c, O.data_ptr(), n_ent, P.data_ptr(), n_ent,
                                               _flags(rt, smode) | rt._lib.RTK_SCORE_KERNEL_WS,
                                               torch.cuda.current_stream().cuda_stream), "ws")
        torch.cuda.synchronize()
        n_sat = int(((P == 1.0) | (P == 0.0)).sum())
        assert n_sat > 0                                   # the saturated branch is exercised
        P64 = P.double().cpu()
        ds.label_smoothing = e
        y = ds.dense(ids, torch.float64)
        ref_rows = -(y * P64.log().clamp_min(-100.0) + (1 - y) * (1 - P64).log().clamp_min(-100.0)).sum(1)
        dZ = (P64 - y) * ((P64 > 0) & (P64 < 1))
        ref_dv = dZ @ O.double().cpu()
        ref_gO = dZ.T @ v.double().cpu()
        e_rows = ((rows.cpu() - ref_rows).abs() / ref_rows.abs()).max().item()
        e_dv = (dv.double().cpu() - ref_dv).abs().max().item() / ref_dv.abs().max().item()
        e_gO = (gO.double().cpu() - ref_gO).abs().max().item() / ref_gO.abs().max().item()
        print(f"c {c} {smode} eps {e}: {n_sat} saturated; rel err rows {e_rows:.2e} dv {e_dv:.2e} gO {e_gO:.2e}")
        assert e_rows <= 2e-6 and e_dv <= 2e-4 and e_gO <= 2e-4
    # eps = 0: the loss rows of the matrix-free ranking (same fragments, another summation order)
    _, bce = rt.rank_1vN(core, R, S, O, h, r, h, flt=flt, want_bce=True, sigmoid_mode=smode)
    assert ((rows - bce).abs() / bce.abs()).max().item() <= 1e-5


def test_accuracy_relative_to_the_matrix_form(rt):
    """WN18RR train batch of 512 at rank (10, 200, 200): for each gradient the max-norm error against float64 of the
    matrix-free form is at most twice the matrix form's (floor 1e-6 max|ref|)."""
    from r_tucker_amd.data import Data, KG_dataset
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    train = KG_dataset(data, data.train_data, label_smoothing=0.1)
    n_ent, n_rel, rank = len(data.entities), len(data.relations), (10, 200, 200)
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, 7)
    core = (core * 0.4).astype(np.float32)
    ids = np.arange(1000, 1512)
    f = train.features[ids]
    h, r = torch.from_numpy(f[:, 0].copy()), torch.from_numpy(f[:, 1].copy())
    t64 = [torch.from_numpy(x).double() for x in (core, R, S, O)]
    assert orc.logits_ref(*t64, h, r).abs().max().item() < 12.0
    ref = orc.bce_loss_grads_ref(*t64, h, r, train.dense_targets(ids).double())
    flt = rt.DeviceFilter(train, "cuda")
    errs = {}
    for form in (False, True):
        ps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (core, R, S, O)]
        loss = rt.bce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(), label_smoothing=0.1,
                               matrix_free=form)
        assert abs(loss.item() - ref[0].item()) <= 2e-6 * max(1.0, abs(ref[0].item()))
        loss.backward()
        errs[form] = [(p.grad.double().cpu() - e).abs().max().item() for p, e in zip(ps, ref[1:])]
    for name, e, em, es in zip(("core", "R", "S", "O"), ref[1:], errs[False], errs[True]):
        print(f"g_{name}: max|ref| {e.abs().max().item():.3e}  err matrix {em:.3e}  err matrix-free {es:.3e}")
    for e, em, es in zip(ref[1:], errs[False], errs[True]):
        assert es <= 2.0 * max(em, 1e-6 * e.abs().max().item())


def test_no_batch_times_entities_allocation(rt):
    """N = 400 000, B = 2048 (the matrix would be 3.3 GB): forward + backward raise the peak by less than B N 4 / 8."""
    n_ent, n_rel, B, rank = 400_000, 7, 2048, (4, 64, 64)
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, 5)
    core = (core * 0.4).astype(np.float32)
    ds, ids = _batch(n_ent, n_rel, B, 5, 0.1, n_pairs=B)
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (core, R, S, O)]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=0.1, matrix_free=True)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.1f} MB; the matrix is {B * n_ent * 4 / 1e6:.0f} MB")
    assert rise < B * n_ent * 4 // 8
    # blockwise float64 reference: the loss over every query (the sampled queries among them), gO on 1000 sampled rows
    with torch.no_grad():
        c64, R64, S64, O64 = [p.detach().double() for p in ps]
        v = orc.query_vectors_ref(c64, R64, S64, h, r)
        tot, zmax = 0.0, 0.0
        y0 = 0.1 / n_ent
        for lo in range(0, B, 64):
            z = v[lo:lo + 64] @ O64.T
            zmax = max(zmax, z.abs().max().item())
            y = torch.full_like(z, y0)
            for row, i in enumerate(ids[lo:lo + 64]):
                y[row, torch.from_numpy(ds._obj[ds._ptr[i]:ds._ptr[i + 1]]).cuda()] = 0.9 + y0
            tot += torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="sum").item()
        assert zmax < 12.0
        ref_loss = tot / (B * n_ent)
        assert abs(loss.item() - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))
        rows_s = torch.from_numpy(np.random.default_rng(6).permutation(n_ent)[:1000]).cuda()
        rows_s[:8] = torch.from_numpy(ds._obj[:8]).cuda()                 # some rows that positives touch
        dZ = torch.sigmoid(v @ O64[rows_s].T) - y0
        for row, i in enumerate(ids):
            objs = torch.from_numpy(ds._obj[ds._ptr[i]:ds._ptr[i + 1]]).cuda()
            hit = (rows_s[None, :] == objs[:, None]).any(0)
            dZ[row, hit] -= 0.9
        ref_gO = dZ.T @ v / (B * n_ent)
        err = (ps[3].grad[rows_s].double() - ref_gO).abs().max().item()
        print(f"gO on 1000 rows: err {err:.3e} of max {ref_gO.abs().max().item():.3e}")
        assert err <= 2e-4 * ref_gO.abs().max().item() + 1e-12


def test_determinism_and_independence_of_the_batch_order(rt):
    n_ent, n_rel, B, rank, eps = 3003, 7, 70, (5, 100, 100), 0.1
    core, R, S, O = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, rank, 47)]
    ds, ids = _batch(n_ent, n_rel, B, 47, eps, empty=True)
    flt = rt.DeviceFilter(ds, "cuda")
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    runs = []
    for _ in range(2):
        ps = [x.clone().requires_grad_(True) for x in (core, R, S, O)]
        loss = rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=eps, matrix_free=True)
        loss.backward()
        runs.append([loss.detach()] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    slot = flt.slot_of_item[idc].contiguous()
    max_pos = B * flt.max_list
    rows, dv, gO, _, _ = _abi(rt, core, R, S, O, h, r, slot, flt, eps, "fast", max_pos)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(B)).cuda()
    rows_p, dv_p, gO_p, _, _ = _abi(rt, core, R, S, O, h[perm], r[perm], slot[perm].contiguous(), flt, eps, "fast", max_pos)
    assert torch.equal(rows_p, rows[perm]) and torch.equal(dv_p, dv[perm])
    assert (gO_p - gO).abs().max().item() <= 1e-6 * gO.abs().max().item()


def test_refusals(rt):
    lib = rt._lib.load()
    n_ent, n_rel, B = 500, 5, 16
    ds, ids = _batch(n_ent, n_rel, B, 3, 0.1)
    flt = rt.DeviceFilter(ds, "cuda")
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    for c in (212, 224):
        ps = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, (3, c, c), 3)]
        with pytest.raises(RuntimeError, match="c <= 208"):
            rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=0.1, matrix_free=True)
    ps = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, (3, 32, 32), 3)]
    with pytest.raises(RuntimeError, match="float32 operands only"):
        rt.bce_loss_1vN(*[p.bfloat16() for p in ps], h, r, flt, idc, label_smoothing=0.1, matrix_free=True)
    # the ABI: unsupported rank, short / misaligned workspace, unknown flags -- nothing is enqueued
    c, sp = 32, torch.cuda.current_stream().cuda_stream
    core, R, S, O = ps
    v, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    slot = flt.slot_of_item[idc].contiguous()
    need = lib.rtk_bce_stream_workspace_bytes(B, n_ent, c, 64)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    rows = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    gO = torch.full((n_ent, c), -7.0, device="cuda")
    sc = torch.ones(1, device="cuda")
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    fl = _flags(rt, "fast")

    def rows_call(c=c, ws_ptr=ws.data_ptr(), nbytes=need, flags=fl):
        return lib.rtk_bce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, 0.1, flags, rows.data_ptr(), None,
                                           ws_ptr, nbytes, sp)

    def go_call(c=c, ws_ptr=ws.data_ptr(), nbytes=need, flags=fl):
        return lib.rtk_bce_stream_grad_o_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, 64, 0.1, flags,
                                             sc.data_ptr(), gO.data_ptr(), ws_ptr, nbytes, sp)
    for call in (rows_call, go_call):
        assert call(c=212) == -3 and b"208" in lib.rtk_last_error_string()
        assert call(c=224) == -3
        assert call(nbytes=255) == -1 and b"workspace" in lib.rtk_last_error_string()
        assert call(ws_ptr=ws.data_ptr() + 16) == -1 and b"aligned" in lib.rtk_last_error_string()
        assert call(flags=fl | 0x40) == -1 and b"unknown flags" in lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((gO == -7.0).all())
    # an out-of-range subject id follows index_check
    bad = h.clone()
    bad[0] = n_ent + 5
    with pytest.raises(IndexError):
        rt.bce_loss_1vN(core, R, S, O, bad, r, flt, idc, label_smoothing=0.1, matrix_free=True)
    with rt.index_check("deferred"):
        rt.bce_loss_1vN(core, R, S, O, bad, r, flt, idc, label_smoothing=0.1, matrix_free=True)
        with pytest.raises(IndexError):
            rt.check_device_errors()
    # batch == 0: a zero loss of the right dtype, zero gradients
    leaves = [p.clone().requires_grad_(True) for p in ps]
    loss = rt.bce_loss_1vN(*leaves, h[:0], r[:0], flt, idc[:0], label_smoothing=0.1, matrix_free=True)
    assert loss.dtype == torch.float32 and loss.item() == 0.0
    loss.backward()
    assert all(p.grad is not None and not p.grad.any() for p in leaves)


def test_no_grad_computes_no_dv_and_backward_twice(rt):
    n_ent, n_rel, B = 3001, 7, 48
    ds, ids = _batch(n_ent, n_rel, B, 9, 0.1)
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gen.make_params(n_ent, n_rel, (5, 32, 32), 9)]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    loss = rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=0.1, matrix_free=True)
    with torch.no_grad():
        assert rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=0.1, matrix_free=True).item() == loss.item()
    loss.backward(retain_graph=True)
    first = [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    loss.backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(first, ps))
    # only O needs a gradient / O needs none
    for want_o in (True, False):
        qs = [p.detach().clone().requires_grad_(want_o == (i == 3)) for i, p in enumerate(ps)]
        rt.bce_loss_1vN(*qs, h, r, flt, idc, label_smoothing=0.1, matrix_free=True).backward()
        for a, q in zip(first, qs):
            assert (q.grad is None) if not q.requires_grad else torch.equal(a, q.grad)


def test_abi_calls_are_graph_capturable(rt):
    """Forward and backward ABI calls captured in one graph and replayed once onto a drained stream: the eager bits."""
    lib = rt._lib.load()
    n_ent, n_rel, B, c, eps = 4099, 9, 96, 64, 0.1
    core, R, S, O = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, (5, c, c), 12)]
    ds, ids = _batch(n_ent, n_rel, B, 12, eps)
    flt = rt.DeviceFilter(ds, "cuda")
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    slot = flt.slot_of_item[torch.from_numpy(ids).cuda()].contiguous()
    max_pos = B * flt.max_list
    rows_e, dv_e, gO_e, v, qp = _abi(rt, core, R, S, O, h, r, slot, flt, eps, "fast", max_pos, scale=0.5)
    ws = torch.zeros(lib.rtk_bce_stream_workspace_bytes(B, n_ent, c, max_pos), dtype=torch.uint8, device="cuda")
    rows = torch.zeros(B, dtype=torch.float64, device="cuda")
    dv = torch.zeros((B, c), device="cuda")
    gO = torch.zeros((n_ent, c), device="cuda")
    sc = torch.tensor([0.5], device="cuda")
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    fl = _flags(rt, "fast")

    def both():
        sp = torch.cuda.current_stream().cuda_stream
        rt._lib.check(lib.rtk_bce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, eps, fl, rows.data_ptr(),
                                                  dv.data_ptr(), ws.data_ptr(), ws.numel(), sp), "rows")
        rt._lib.check(lib.rtk_bce_stream_grad_o_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, max_pos,
                                                    eps, fl, sc.data_ptr(), gO.data_ptr(), ws.data_ptr(), ws.numel(), sp),
                      "grad_o")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                             # first use outside the capture (function attributes)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for t in (rows, dv, gO):
        t.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(rows, rows_e) and torch.equal(dv, dv_e) and torch.equal(gO, gO_e)


def test_twenty_adam_steps_agree_with_the_matrix_form(rt):
    n_ent, n_rel, B, rank = 3000, 7, 128, (5, 32, 32)
    ds, _ = _batch(n_ent, n_rel, B, 21, 0.1, n_pairs=600)
    flt = rt.DeviceFilter(ds, "cuda")
    init = gen.make_params(n_ent, n_rel, rank, 21)
    final = {}
    for form in (False, True):
        ps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in init]
        opt = torch.optim.Adam(ps, lr=1e-2)
        rng = np.random.default_rng(22)
        for _ in range(20):
            ids = rng.permutation(600)[:B]
            h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
            r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
            opt.zero_grad(set_to_none=True)
            loss = rt.bce_loss_1vN(*ps, h, r, flt, torch.from_numpy(ids).cuda(), label_smoothing=0.1, matrix_free=form)
            loss.backward()
            opt.step()
        final[form] = loss.item()
    print(f"loss after 20 steps: matrix {final[False]:.8g}  matrix-free {final[True]:.8g}")
    assert abs(final[True] - final[False]) <= 1e-3 * abs(final[False])
