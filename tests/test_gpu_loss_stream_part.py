"""The matrix-free 1-vs-all BCE loss on blocks of entity rows (rtk_bce_stream_rows_part_f32 /
rtk_bce_stream_grad_o_part_f32 behind bce_loss_block_1vN and ShardedEntityScorer.bce_loss_1vN): one block against the
whole-matrix entry points bit for bit, partitions against float64, the oracle through autograd, the global smoothing
term, world size 1, peak memory, determinism, graph capture, a short optimizer run and two real ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                       # a rank of test_two_real_ranks: a fresh process, no conftest
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import gen  # noqa: E402
from oracle import score_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _cuts(n_ent, parts):
    return [n_ent * i // parts for i in range(parts + 1)]


def _abi_whole(rt, qp, v, O, slot, flt, eps, mode, max_pos, scale=1.0):
    """rows, dv, gO of the whole-matrix entry points on fresh buffers."""
    lib = rt._lib.load()
    B, (N, c) = v.shape[0], O.shape
    ws = torch.zeros(lib.rtk_bce_stream_workspace_bytes(B, N, c, max_pos), dtype=torch.uint8, device="cuda")
    rows = torch.empty(B, dtype=torch.float64, device="cuda")
    dv = torch.empty((B, c), dtype=torch.float32, device="cuda")
    gO = torch.empty((N, c), dtype=torch.float32, device="cuda")
    sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    rt._lib.check(lib.rtk_bce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), N, *csr, eps, _flags(rt, mode),
                                              rows.data_ptr(), dv.data_ptr(), ws.data_ptr(), ws.numel(), sp), "rows")
    rt._lib.check(lib.rtk_bce_stream_grad_o_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), N, *csr, max_pos, eps,
                                                _flags(rt, mode), sc.data_ptr(), gO.data_ptr(), ws.data_ptr(), ws.numel(),
                                                sp), "grad_o")
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0
    return rows, dv, gO


def _abi_part(rt, qp, v, O_blk, col0, n_ent, slot, flt, eps, mode, max_pos, scale=1.0, out=None, ws=None, sc=None):
    """rows, dv, gO of the block entry points for rows [col0, col0 + n_local), on fresh buffers unless given."""
    lib = rt._lib.load()
    B, (n_local, c) = v.shape[0], O_blk.shape
    assert O_blk.is_contiguous() and 0 <= col0 and col0 + n_local <= n_ent          # bounds before any launch
    if ws is None:
        ws = torch.zeros(lib.rtk_bce_stream_part_workspace_bytes(B, n_local, c, max_pos), dtype=torch.uint8, device="cuda")
    rows, dv, gO = out or (torch.empty(B, dtype=torch.float64, device="cuda"),
                           torch.empty((B, c), dtype=torch.float32, device="cuda"),
                           torch.empty((n_local, c), dtype=torch.float32, device="cuda"))
    if sc is None:
        sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    rt._lib.check(lib.rtk_bce_stream_rows_part_f32(qp.data_ptr(), B, c, O_blk.data_ptr(), n_local, col0, n_ent, *csr, eps,
                                                   _flags(rt, mode), rows.data_ptr(), dv.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), sp), "rows_part")
    rt._lib.check(lib.rtk_bce_stream_grad_o_part_f32(qp.data_ptr(), v.data_ptr(), B, c, O_blk.data_ptr(), n_local, col0,
                                                     n_ent, *csr, max_pos, eps, _flags(rt, mode), sc.data_ptr(),
                                                     gO.data_ptr(), ws.data_ptr(), ws.numel(), sp), "grad_o_part")
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0
    return rows, dv, gO


def _setup(rt, n_ent, rank, B, seed, eps, core_scale=0.4, n_rel=7, ds_ids=None, **kw):
    """Device operands, queries, filter, slots and max_pos of one synthetic case."""
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, seed)
    core = (core * core_scale).astype(np.float32)
    ds, ids = ds_ids if ds_ids is not None else _batch(n_ent, n_rel, B, seed, eps, **kw)
    flt = rt.DeviceFilter(ds, "cuda")
    host = [torch.from_numpy(x) for x in (core, R, S, O)]
    dev = [x.cuda() for x in host]
    h = torch.from_numpy(ds.features[ids, 0].copy())
    r = torch.from_numpy(ds.features[ids, 1].copy())
    slot = flt.slot_of_item[torch.from_numpy(ids).cuda()].contiguous()
    return host, dev, ds, ids, flt, h, r, slot, B * max(1, flt.max_list)


@pytest.mark.parametrize("smode", ["fast", "exact"])
@pytest.mark.parametrize("c,B,n_ent", [(200, 70, 3003), (208, 33, 3003)])
def test_one_block_is_the_whole_matrix_call(rt, c, B, n_ent, smode):
    """col0 = 0, n_local = n_ent: the bits of rtk_bce_stream_rows_f32 / rtk_bce_stream_grad_o_f32."""
    _, (core, R, S, O), ds, ids, flt, h, r, slot, max_pos = _setup(rt, n_ent, (5, c, c), B, 41, 0.1, empty=True)
    v, qp = rt.query_vectors(core, R, S, h.cuda(), r.cuda(), packed=True)
    whole = _abi_whole(rt, qp, v, O, slot, flt, 0.1, smode, max_pos, scale=0.25)
    part = _abi_part(rt, qp, v, O, 0, n_ent, slot, flt, 0.1, smode, max_pos, scale=0.25)
    for name, a, b in zip(("rows", "dv", "gO"), whole, part):
        assert torch.equal(a, b), name


def _float64_reference(host, ds, ids, h, r, scale=1.0):
    """rows, dv, gO in float64 on the host, from float64 probabilities; the float64 logits' largest magnitude."""
    c64, R64, S64, O64 = [x.double() for x in host]
    z = orc.logits_ref(c64, R64, S64, O64, h, r)
    v64 = orc.query_vectors_ref(c64, R64, S64, h, r)
    P64 = torch.sigmoid(z)
    y = ds.dense(ids, torch.float64)
    ref_rows = -(y * P64.log() + (1 - y) * (1 - P64).log()).sum(1)
    dZ = P64 - y
    return ref_rows, dZ @ O64, dZ.T @ (v64 * scale), z.abs().max().item()


def _low_objects_batch(n_ent, n_lo, n_rel, B, seed, eps):
    """A pair table whose known objects all lie below n_lo: a block at or above n_lo owns no positive of any query."""
    ds, ids = _batch(n_lo, n_rel, B, seed, eps, empty=True)
    ds.n_ent = n_ent
    assert ds._obj.max() < n_lo
    return ds, ids


PARTITIONS = {
    "two blocks, cut at 1501": lambda n: [0, 1501, n],
    "eight near-equal blocks": lambda n: _cuts(n, 8),
    "a one-row block": lambda n: [0, 1000, 1001, n],
    "a block without positives": lambda n: [0, 2000, n],
}


@pytest.mark.parametrize("smode", ["fast", "exact"])
@pytest.mark.parametrize("name", list(PARTITIONS))
def test_partitions_add_up(rt, name, smode):
    """Rows and dv summed, gO concatenated over a partition of [0, n_ent) against float64: the error is at most twice
    that of the whole-matrix call on the same operands (floor 1e-6 max|reference|), on unsaturated scores."""
    n_ent, n_rel, B, c, eps = 3003, 7, 70, 200, 0.1
    cuts = PARTITIONS[name](n_ent)
    assert cuts[0] == 0 and cuts[-1] == n_ent and all(a < b for a, b in zip(cuts, cuts[1:]))
    ds_ids = _low_objects_batch(n_ent, 2000, n_rel, B, 41, eps) if "without positives" in name else None
    host, (core, R, S, O), ds, ids, flt, h, r, slot, max_pos = _setup(rt, n_ent, (5, c, c), B, 41, eps, empty=True,
                                                                       ds_ids=ds_ids)
    ref_rows, ref_dv, ref_gO, zmax = _float64_reference(host, ds, ids, h, r)
    assert zmax < 12.0                                     # no saturation hides in the comparison
    v, qp = rt.query_vectors(core, R, S, h.cuda(), r.cuda(), packed=True)
    w_rows, w_dv, w_gO = _abi_whole(rt, qp, v, O, slot, flt, eps, smode, max_pos)
    rows = torch.zeros(B, dtype=torch.float64, device="cuda")
    dv = torch.zeros((B, c), dtype=torch.float64, device="cuda")
    blocks = []
    for lo, hi in zip(cuts, cuts[1:]):
        b_rows, b_dv, b_gO = _abi_part(rt, qp, v, O[lo:hi], lo, n_ent, slot, flt, eps, smode, max_pos)
        rows += b_rows
        dv += b_dv.double()
        blocks.append(b_gO)
    gO = torch.cat(blocks)
    print(f"{name} ({smode}): gO blocks bit-equal to the whole-matrix gO: {torch.equal(gO, w_gO)}; "
          f"rows bit-equal: {torch.equal(rows, w_rows)}")
    for what, got, whole, ref in (("rows", rows, w_rows, ref_rows), ("dv", dv, w_dv, ref_dv), ("gO", gO, w_gO, ref_gO)):
        e_part = (got.double().cpu() - ref).abs().max().item()
        e_whole = (whole.double().cpu() - ref).abs().max().item()
        top = ref.abs().max().item()
        print(f"  {what}: max|ref| {top:.3e}  err whole {e_whole:.3e}  err partition {e_part:.3e}")
        assert e_part <= 2.0 * max(e_whole, 1e-6 * top), what


@pytest.mark.parametrize("mode", ["asym", "sym"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_and_gradients_against_oracle_over_three_blocks(rt, mode, eps):
    """The cases and bounds of test_gpu_loss_stream.py::test_loss_and_gradients_against_oracle with the loss and the
    gradients assembled from bce_loss_block_1vN(all_reduce=None) over 3 blocks; O_loc is a slice of the (shared) matrix,
    so autograd scatters the block gradients (and adds gS in the symmetric case)."""
    n_ent, n_rel, rank, B, seed = 3001, 7, (5, 32, 32), 48, 41
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, seed, shared=(mode == "sym"))
    ds, ids = _batch(n_ent, n_rel, B, seed, eps)
    h = torch.from_numpy(ds.features[ids, 0].copy())
    r = torch.from_numpy(ds.features[ids, 1].copy())
    tc, tR, tS, tO = [torch.from_numpy(x) for x in (core, R, S, O)]
    ref = orc.bce_loss_grads_ref(tc, tR, tS, tO, h, r, ds.dense(ids), shared=(mode == "sym"))
    flt = rt.DeviceFilter(ds, "cuda")
    dc, dR, dS = [x.clone().cuda().requires_grad_(True) for x in (tc, tR, tS)]
    dO = dS if mode == "sym" else tO.clone().cuda().requires_grad_(True)
    idc = torch.from_numpy(ids).cuda()
    loss = 0.0
    for lo, hi in zip([0, 1000, 2001], [1000, 2001, n_ent]):
        loss = loss + rt.bce_loss_block_1vN(dc, dR, dS, dO[lo:hi], lo, n_ent, h.cuda(), r.cuda(), flt, idc,
                                            label_smoothing=eps)
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


def _smoothing_case():
    """n_ent 64 in two blocks of 32, negatives only: host operands, the table, and float64 loss / dv / gO with the
    smoothing term eps / n_ent (right) and eps / n_local (wrong)."""
    n_ent, n_rel, B, rank, eps = 64, 7, 20, (3, 16, 16), 0.5
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, 41)
    host = [torch.from_numpy(x) for x in ((core * 0.4).astype(np.float32), R, S, O)]
    rng = np.random.default_rng(41)
    pairs = [(int(s), int(r)) for s, r in zip(rng.permutation(n_ent)[:B + 1], rng.integers(0, n_rel, B + 1))]
    ds = _Pairs(pairs, [[] for _ in range(B)] + [[5]], n_ent, eps)       # the batch's queries know no object
    ids = np.arange(B, dtype=np.int64)
    h = torch.from_numpy(ds.features[ids, 0].copy())
    r = torch.from_numpy(ds.features[ids, 1].copy())
    c64, R64, S64, O64 = [x.double() for x in host]
    z = orc.logits_ref(c64, R64, S64, O64, h, r)
    assert z.abs().max().item() < 12.0
    v64 = orc.query_vectors_ref(c64, R64, S64, h, r)
    P = torch.sigmoid(z)
    out = {}
    for key, t0 in (("right", eps / n_ent), ("wrong", eps / 32)):
        loss = -(t0 * P.log() + (1 - t0) * (1 - P).log()).sum().item() / (B * n_ent)
        out[key] = (loss, (P - t0) @ O64, (P - t0).T @ v64)
    return host, ds, ids, h, r, eps, out


def test_the_smoothing_term_is_global(rt):
    """eps / n_local in place of eps / n_ent would be invisible at n_ent 3001; here (n_ent 64, eps 0.5) it moves the
    float64 loss, dv and gO by at least 10 x the bounds they are then held to."""
    host, ds, ids, h, r, eps, f64 = _smoothing_case()
    n_ent, B = 64, 20
    (l_ok, dv_ok, gO_ok), (l_bad, dv_bad, gO_bad) = f64["right"], f64["wrong"]
    b_loss, b_dv, b_gO = 2e-6 * max(1.0, abs(l_ok)), 2e-4 * dv_ok.abs().max().item(), 2e-4 * gO_ok.abs().max().item()
    d_loss, d_dv, d_gO = abs(l_bad - l_ok), (dv_bad - dv_ok).abs().max().item(), (gO_bad - gO_ok).abs().max().item()
    print(f"a wrong term moves: loss {d_loss:.3e} ({d_loss / b_loss:.1f} x its bound), dv {d_dv / b_dv:.1f} x, "
          f"gO {d_gO / b_gO:.1f} x")
    assert d_loss >= 10 * b_loss and d_dv >= 10 * b_dv and d_gO >= 10 * b_gO
    flt = rt.DeviceFilter(ds, "cuda")
    core, R, S, O = [x.cuda() for x in host]
    slot = flt.slot_of_item[torch.from_numpy(ids).cuda()].contiguous()
    v, qp = rt.query_vectors(core, R, S, h.cuda(), r.cuda(), packed=True)
    parts = [_abi_part(rt, qp, v, O[lo:lo + 32], lo, n_ent, slot, flt, eps, "fast", B) for lo in (0, 32)]
    loss = (parts[0][0] + parts[1][0]).sum().item() / (B * n_ent)
    dv = (parts[0][1].double() + parts[1][1].double()).cpu()
    gO = torch.cat([parts[0][2], parts[1][2]]).double().cpu()
    print(f"loss {loss:.9g} ref {l_ok:.9g}; dv err {(dv - dv_ok).abs().max().item():.3e} (bound {b_dv:.3e}); "
          f"gO err {(gO - gO_ok).abs().max().item():.3e} (bound {b_gO:.3e})")
    assert abs(loss - l_ok) <= b_loss
    assert (dv - dv_ok).abs().max().item() <= b_dv + 1e-9
    assert (gO - gO_ok).abs().max().item() <= b_gO + 1e-9


def test_world_size_one_is_the_unsharded_call(rt):
    """ShardedEntityScorer without a process group: the bits of bce_loss_1vN(matrix_free=True), loss and gradients."""
    n_ent, B, eps = 3001, 48, 0.1
    _, dev, ds, ids, flt, h, r, _, _ = _setup(rt, n_ent, (5, 32, 32), B, 41, eps, core_scale=1.0)
    idc = torch.from_numpy(ids).cuda()
    runs = []
    for sharded in (False, True):
        ps = [x.clone().requires_grad_(True) for x in dev]
        if sharded:
            sc = rt.ShardedEntityScorer(n_ent)
            assert sc.world == 1 and sc.shards.n_loc == n_ent
            loss = sc.bce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, idc, label_smoothing=eps)
        else:
            loss = rt.bce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, idc, label_smoothing=eps, matrix_free=True)
        (loss * 3.0).backward()
        runs.append([loss.detach()] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_no_batch_times_block_allocation(rt):
    """Rows [300 000, 400 000) of n_ent 400 000, B 2048 (the block's scores would be 819 MB): forward + backward raise
    the peak by less than B n_local 4 / 8.  Only the block of O and the first 65 536 rows of S are on the device."""
    n_ent, n_rel, B, rank, eps = 400_000, 7, 2048, (4, 64, 64), 0.1
    lo, hi, n_subj = 300_000, 400_000, 65_536
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, 5)
    core = (core * 0.4).astype(np.float32)
    rng = np.random.default_rng(5)
    pairs = [(int(s), int(r_)) for s, r_ in zip(rng.permutation(n_subj)[:B], rng.integers(0, n_rel, B))]
    ds = _Pairs(pairs, [rng.integers(0, n_ent, rng.integers(1, 9)).tolist() for _ in pairs], n_ent, eps)
    ids = rng.permutation(B).astype(np.int64)
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [torch.from_numpy(np.ascontiguousarray(x)).cuda().requires_grad_(True) for x in (core, R, S[:n_subj], O[lo:hi])]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = rt.bce_loss_block_1vN(*ps, lo, n_ent, h, r, flt, idc, label_smoothing=eps)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.1f} MB; the block's scores are {B * (hi - lo) * 4 / 1e6:.0f} MB")
    assert rise < B * (hi - lo) * 4 // 8
    assert ps[3].grad.shape == (hi - lo, 64) and ps[2].grad.shape == (n_subj, 64)
    with torch.no_grad():                                  # the block's share of the loss, blockwise in float64
        c64, R64, S64, O64 = [p.detach().double() for p in ps]
        v = orc.query_vectors_ref(c64, R64, S64, h, r)
        tot, zmax, y0, n_own = 0.0, 0.0, eps / n_ent, 0
        for q0 in range(0, B, 64):
            z = v[q0:q0 + 64] @ O64.T
            zmax = max(zmax, z.abs().max().item())
            y = torch.full_like(z, y0)
            for row, i in enumerate(ids[q0:q0 + 64]):
                objs = ds._obj[ds._ptr[i]:ds._ptr[i + 1]]
                own = objs[(objs >= lo) & (objs < hi)] - lo
                n_own += len(own)
                y[row, torch.from_numpy(own).cuda()] = (1 - eps) + y0
            tot += torch.nn.functional.binary_cross_entropy_with_logits(z, y, reduction="sum").item()
        assert zmax < 12.0 and n_own > 100                 # the block owns positives
        ref_share = tot / (B * n_ent)
        print(f"loss share {loss.item():.9g} ref {ref_share:.9g}")
        assert abs(loss.item() - ref_share) <= 2e-6 * max(1.0, abs(ref_share))


def test_determinism_graph_capture_and_no_grad(rt):
    n_ent, n_rel, B, c, eps = 4099, 9, 96, 64, 0.1
    lo, hi = 1033, 3011
    _, (core, R, S, O), ds, ids, flt, h, r, slot, max_pos = _setup(rt, n_ent, (5, c, c), B, 12, eps, core_scale=1.0,
                                                                   n_rel=n_rel)
    h, r, idc = h.cuda(), r.cuda(), torch.from_numpy(ids).cuda()
    O_blk = O[lo:hi].contiguous()
    # two calls give the same bits
    runs = []
    for _ in range(2):
        ps = [x.clone().requires_grad_(True) for x in (core, R, S, O_blk)]
        loss = rt.bce_loss_block_1vN(*ps, lo, n_ent, h, r, flt, idc, label_smoothing=eps)
        loss.backward()
        runs.append([loss.detach()] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # the two ABI calls captured in one graph replay to the eager result
    lib = rt._lib.load()
    v, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    eager = _abi_part(rt, qp, v, O_blk, lo, n_ent, slot, flt, eps, "fast", max_pos, scale=0.5)
    ws = torch.zeros(lib.rtk_bce_stream_part_workspace_bytes(B, hi - lo, c, max_pos), dtype=torch.uint8, device="cuda")
    out = (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros((B, c), device="cuda"),
           torch.zeros((hi - lo, c), device="cuda"))

    half = torch.tensor([0.5], device="cuda")

    def both():
        _abi_part(rt, qp, v, O_blk, lo, n_ent, slot, flt, eps, "fast", max_pos, out=out, ws=ws, sc=half)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                             # first use outside the capture (function attributes)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for t in out:
        t.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    # no_grad: the same loss, no dv; a core gradient cannot be asked for afterwards
    ps = [x.clone().requires_grad_(True) for x in (core, R, S, O_blk)]
    with torch.no_grad():
        assert rt.bce_loss_block_1vN(*ps, lo, n_ent, h, r, flt, idc, label_smoothing=eps).item() == runs[0][0].item()
    fn = rt.ops._BceLossBlock
    args = (slot, flt.pair_ptr, flt.pair_obj, eps, None, max_pos, False, lo, n_ent, None, rt.ops._HipBlockLoss)
    loss = fn.apply(*ps, h, r, *args)                     # the DV = false instantiation, as under no_grad
    assert loss.item() == runs[0][0].item()
    with pytest.raises(RuntimeError, match="dv was not computed"):
        loss.backward()
    # only O_loc wants a gradient: no dv is computed and its gradient has the bits of the full call
    qs = [x.clone().requires_grad_(i == 3) for i, x in enumerate((core, R, S, O_blk))]
    rt.bce_loss_block_1vN(*qs, lo, n_ent, h, r, flt, idc, label_smoothing=eps).backward()
    assert torch.equal(qs[3].grad, runs[0][4]) and qs[0].grad is None


def test_twenty_adam_steps_on_four_blocks_agree_with_the_unsharded_form(rt):
    n_ent, n_rel, B, rank = 3000, 7, 128, (5, 32, 32)
    ds, _ = _batch(n_ent, n_rel, B, 21, 0.1, n_pairs=600)
    flt = rt.DeviceFilter(ds, "cuda")
    init = gen.make_params(n_ent, n_rel, rank, 21)
    cuts = _cuts(n_ent, 4)
    final = {}
    for blocks in (False, True):
        ps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in init]
        opt = torch.optim.Adam(ps, lr=1e-2)
        rng = np.random.default_rng(22)
        for _ in range(20):
            ids = rng.permutation(600)[:B]
            h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
            r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
            idc = torch.from_numpy(ids).cuda()
            opt.zero_grad(set_to_none=True)
            if blocks:
                loss = sum(rt.bce_loss_block_1vN(*ps[:3], ps[3][lo:hi], lo, n_ent, h, r, flt, idc, label_smoothing=0.1)
                           for lo, hi in zip(cuts, cuts[1:]))
            else:
                loss = rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=0.1, matrix_free=True)
            loss.backward()
            opt.step()
        final[blocks] = loss.item()
    print(f"loss after 20 steps: unsharded {final[False]:.8g}  four blocks {final[True]:.8g}")
    assert abs(final[True] - final[False]) <= 1e-3 * abs(final[False])


# ---- two real ranks ------------------------------------------------------------------------------------------------

def _two_rank_case(rt):
    n_ent, B, eps = 3001, 48, 0.1                          # odd: the last shard has a padding row
    return (n_ent, eps) + _setup(rt, n_ent, (5, 32, 32), B, 41, eps, core_scale=1.0)


def _rank_main(rank, port, out_path):
    """One rank of world size 2 over RCCL: loss and gradients of ShardedEntityScorer.bce_loss_1vN into an .npz."""
    import torch.distributed as dist
    import r_tucker_amd as rt
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=2)
    try:
        n_ent, eps, _, dev, ds, ids, flt, h, r, _, _ = _two_rank_case(rt)
        sc = rt.ShardedEntityScorer(n_ent)
        ps = [x.clone().requires_grad_(True) for x in dev[:3]] + [sc.local_block(dev[3]).requires_grad_(True)]
        loss = sc.bce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(), label_smoothing=eps)
        (loss * 3.0).backward()
        torch.cuda.synchronize()
        np.savez(out_path, loss=loss.item(), **{f"g{i}": p.grad.cpu().numpy() for i, p in enumerate(ps)})
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_real_ranks(rt, tmp_path):
    """World size 2 over RCCL (each rank a fresh child process) equals the world-size-1 result within the bounds of the
    oracle test; the gradients of core, R and S are equal on the two ranks."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"          # dmabuf IPC (RCCL across processes)
    outs = [str(tmp_path / f"rank{k}.npz") for k in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(k), str(port), outs[k]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), [l[-3000:] for l in logs]
    got = [np.load(o) for o in outs]
    n_ent, eps, _, dev, ds, ids, flt, h, r, _, _ = _two_rank_case(rt)
    ps = [x.clone().requires_grad_(True) for x in dev]
    loss = rt.ShardedEntityScorer(n_ent).bce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(),
                                                      label_smoothing=eps)
    (loss * 3.0).backward()
    ref = [p.grad.cpu().numpy() for p in ps]
    n_loc = -(-n_ent // 2)
    for k in range(2):
        assert abs(float(got[k]["loss"]) - loss.item()) <= 2e-6 * max(1.0, abs(loss.item()))
        for i in range(3):
            assert np.abs(got[k][f"g{i}"] - ref[i]).max() <= 2e-4 * np.abs(ref[i]).max() + 1e-9
    for i in range(3):
        assert np.array_equal(got[0][f"g{i}"], got[1][f"g{i}"])
    gO = np.concatenate([got[0]["g3"], got[1]["g3"]])
    assert gO.shape == (2 * n_loc, 32) and not gO[n_ent:].any()       # the padding row's gradient is 0
    assert np.abs(gO[:n_ent] - ref[3]).max() <= 2e-4 * np.abs(ref[3]).max() + 1e-9


if __name__ == "__main__":
    assert sys.argv[1] == "--rank"
    _rank_main(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
