"""The softmax cross-entropy 1-vs-all loss (ce_loss_1vN: rtk_ce_* on stored logits, rtk_ce_stream_* without the (B, N)
matrix) against float64 -- oracle.logits_ref with autograd, then F.cross_entropy on the targets of the definition --
at the bounds of test_gpu_loss_stream.py: loss <= 2e-6 max(1, |ref|), each gradient <= 2e-4 max|ref| + 1e-9 in the
max norm.  Every case multiplies the loss by 3.0 before backward()."""
import math
import os

import numpy as np
import pytest
import torch

import ce_cases
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


def _case(n_ent, rank, B, seed, eps, empty, core_scale=1.0, shared=False, n_rel=7):
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, seed, shared=shared)
    core = (core * core_scale).astype(np.float32)
    ds, ids = ce_cases.batch(n_ent, n_rel, B, seed, eps, empty=empty)
    h = torch.from_numpy(ds.features[ids, 0].copy())
    r = torch.from_numpy(ds.features[ids, 1].copy())
    return [torch.from_numpy(x) for x in (core, R, S, O)], ds, ids, h, r


def _run(rt, params, ds, ids, h, r, eps, matrix_free, shared):
    """(loss, [g_core, g_R, g_S(, g_O)]) of 3.0 * ce_loss_1vN on the device."""
    flt = rt.DeviceFilter(ds, "cuda")
    dc, dR, dS = [x.clone().cuda().requires_grad_(True) for x in params[:3]]
    dO = dS if shared else params[3].clone().cuda().requires_grad_(True)
    loss = rt.ce_loss_1vN(dc, dR, dS, dO, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(), label_smoothing=eps,
                          matrix_free=matrix_free)
    (loss * 3.0).backward()                                    # a non-unit upstream gradient
    return loss, [dc.grad, dR.grad, dS.grad] + ([] if shared else [dO.grad])


def _check(rt, n_ent, rank, B, eps, matrix_free, empty, shared=False, seed=41, core_scale=1.0, loss_tol=None, grad_rel=2e-4):
    params, ds, ids, h, r = _case(n_ent, rank, B, seed, eps, empty, core_scale, shared)
    ref = ce_cases.ce_ref(*params, h, r, ds.targets(ids, eps), shared=shared)
    loss, got = _run(rt, params, ds, ids, h, r, eps, matrix_free, shared)
    tol = 2e-6 * max(1.0, abs(ref[0].item())) if loss_tol is None else loss_tol
    print(f"loss {loss.item():.9g} ref {ref[0].item():.9g} (bound {tol:.3e}); max|z| {ref[-1]:.3f}")
    assert math.isfinite(loss.item())
    assert abs(loss.item() - ref[0].item()) <= tol
    assert len(got) == len(ref) - 2
    for g, e in zip(got, ref[1:-1]):
        e = 3.0 * e
        assert g.shape == e.shape
        err = (g.double().cpu() - e).abs().max().item()
        print(f"grad {tuple(e.shape)}: err {err:.3e} of max {e.abs().max().item():.3e}")
        assert err <= grad_rel * e.abs().max().item() + 1e-9


@pytest.mark.parametrize("matrix_free", [False, True])
@pytest.mark.parametrize("mode", ["asym", "sym"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_both_forms_against_float64(rt, mode, eps, matrix_free):
    _check(rt, 3001, (5, 32, 32), 48, eps, matrix_free, False, shared=(mode == "sym"))


@pytest.mark.parametrize("c,B,n_ent,eps", [(4, 1, 31, 0.1), (100, 33, 3003, 0.1), (100, 1, 3003, 0.1), (200, 70, 3003, 0.1),
                                          (208, 70, 31, 0.1), (208, 33, 3003, 0.1), (4, 70, 3003, 0.1), (200, 1, 31, 0.1),
                                          (100, 33, 3003, 0.0)])
def test_edges_of_the_matrix_free_range(rt, c, B, n_ent, eps):
    """One query with an empty list; B = 1 at N = 3003: more splits than work per split; N = 31: splits that have no
    tile; eps = 0 with the empty list: a row of mass w_d = 0."""
    _check(rt, n_ent, (5, c, c), B, eps, True, True)


@pytest.mark.parametrize("c,a", [(400, 10), (30, 5)])
def test_matrix_form_beyond_the_matrix_free_range(rt, c, a):
    _check(rt, 3003, (a, c, c), 33, 0.1, False, True)


@pytest.mark.parametrize("matrix_free", [False, True])
def test_large_logits(rt, matrix_free):
    """The core scaled so that the float64 reference's max |z| is near 100.  The logit parity bound 2e-5 (1 + |z|) enters
    the lse and the target term once each."""
    n_ent, rank, B, eps, seed = 3003, (5, 64, 64), 33, 0.1, 41
    params, ds, ids, h, r = _case(n_ent, rank, B, seed, eps, True)
    z1 = orc.logits_ref(*[p.double() for p in params], h, r).abs().max().item()
    scale = 100.0 / z1
    params, ds, ids, h, r = _case(n_ent, rank, B, seed, eps, True, core_scale=scale)
    zmax = orc.logits_ref(*[p.double() for p in params], h, r).abs().max().item()
    assert 50.0 <= zmax <= 200.0
    pz = 2 * 2e-5 * (1.0 + zmax)
    _check(rt, n_ent, rank, B, eps, matrix_free, True, core_scale=scale, loss_tol=pz, grad_rel=2e-4 + pz)


def test_no_batch_times_entities_allocation(rt):
    """N = 400 000, B = 2048 (the matrix would be 3.3 GB): forward + backward raise the peak by less than B N 4 / 8."""
    n_ent, n_rel, B, rank, eps = 400_000, 7, 2048, (4, 64, 64), 0.1
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, 5)
    core = (core * 0.4).astype(np.float32)
    ds, ids = ce_cases.batch(n_ent, n_rel, B, 5, eps, n_pairs=B)
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (core, R, S, O)]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = rt.ce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=eps, matrix_free=True)
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.1f} MB; the matrix is {B * n_ent * 4 / 1e6:.0f} MB")
    assert rise < B * n_ent * 4 // 8
    # blockwise float64 reference: the loss over every query, gO on 1000 sampled rows
    with torch.no_grad():
        c64, R64, S64, O64 = [p.detach().double() for p in ps]
        v = orc.query_vectors_ref(c64, R64, S64, h, r)
        y0 = eps / n_ent
        objs = [torch.from_numpy(ds.objects(i)).cuda() for i in ids]
        w = torch.tensor([(1 - eps) * (len(o) > 0) + eps for o in objs], dtype=torch.float64, device="cuda")
        lse = torch.empty(B, dtype=torch.float64, device="cuda")
        tot = 0.0
        for lo in range(0, B, 64):
            z = v[lo:lo + 64] @ O64.T
            lse[lo:lo + 64] = torch.logsumexp(z, 1)
            tot += (w[lo:lo + 64] * lse[lo:lo + 64] - y0 * z.sum(1)).sum().item()
            for row in range(z.shape[0]):
                o = objs[lo + row]
                if len(o):
                    tot -= (1 - eps) / len(o) * z[row, o].sum().item()
        ref_loss = tot / B
        print(f"loss {loss.item():.9g} ref {ref_loss:.9g}")
        assert abs(loss.item() - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))
        rows_s = torch.from_numpy(np.random.default_rng(6).permutation(n_ent)[:1000]).cuda()
        rows_s[:8] = torch.from_numpy(ds._obj[:8]).cuda()                 # some rows that positives touch
        dZ = w[:, None] * torch.exp(v @ O64[rows_s].T - lse[:, None]) - y0
        for row, o in enumerate(objs):
            if len(o):
                hit = (rows_s[None, :] == o[:, None]).any(0)
                dZ[row, hit] -= (1 - eps) / len(o)
        ref_gO = 3.0 * dZ.T @ v / B
        err = (ps[3].grad[rows_s].double() - ref_gO).abs().max().item()
        print(f"gO on 1000 rows: err {err:.3e} of max {ref_gO.abs().max().item():.3e}")
        assert err <= 2e-4 * ref_gO.abs().max().item() + 1e-12


@pytest.mark.parametrize("matrix_free", [False, True])
def test_determinism(rt, matrix_free):
    params, ds, ids, h, r = _case(3003, (5, 100, 100), 70, 47, 0.1, True)
    runs = []
    for _ in range(2):
        loss, grads = _run(rt, params, ds, ids, h, r, 0.1, matrix_free, False)
        runs.append([loss.detach()] + grads)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_grad_runs_the_forward_sweep_only(rt):
    """The loss bits of the grad-enabled forward, and no (B, c) buffer beside the query vectors: after a first call
    (the cached workspace exists) the peak rises by v, the packed planes and B-sized vectors."""
    n_ent, B, c, eps = 3001, 512, 200, 0.1
    params, ds, ids, h, r = _case(n_ent, (5, c, c), B, 9, eps, False, core_scale=0.4)
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [x.cuda().requires_grad_(True) for x in params]
    hc, rc, idc = h.cuda(), r.cuda(), torch.from_numpy(ids).cuda()
    loss = rt.ce_loss_1vN(*ps, hc, rc, flt, idc, label_smoothing=eps, matrix_free=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        quiet = rt.ce_loss_1vN(*ps, hc, rc, flt, idc, label_smoothing=eps, matrix_free=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert not quiet.requires_grad and torch.equal(quiet, loss.detach())
    planes = rt._lib.load().rtk_packed_query_bytes(0, B, c)
    print(f"no_grad peak rise {rise} bytes; v {B * c * 4}, planes {planes}")
    assert rise < B * c * 4 + planes + B * c * 4 // 2


def test_refusals(rt):
    n_ent, n_rel, B = 500, 5, 16
    ds, ids = ce_cases.batch(n_ent, n_rel, B, 3, 0.1)
    flt = rt.DeviceFilter(ds, "cuda")
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    for c in (212, 30):
        ps = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, (3, c, c), 3)]
        with pytest.raises(RuntimeError, match=r"ce_loss_1vN\(matrix_free=True\).*c <= 208"):
            rt.ce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=0.1, matrix_free=True)
    ps = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, (3, 32, 32), 3)]
    for form in (True, False):
        with pytest.raises(RuntimeError, match="float32 operands only"):
            rt.ce_loss_1vN(*[p.bfloat16() for p in ps], h, r, flt, idc, label_smoothing=0.1, matrix_free=form)
    # batch == 0: a zero loss, zero gradients, in both forms
    for form in (True, False):
        leaves = [p.clone().requires_grad_(True) for p in ps]
        loss = rt.ce_loss_1vN(*leaves, h[:0], r[:0], flt, idc[:0], label_smoothing=0.1, matrix_free=form)
        assert loss.dtype == torch.float32 and loss.item() == 0.0
        loss.backward()
        assert all(p.grad is not None and not p.grad.any() for p in leaves)


def test_abi_single_outputs_and_the_max_pos_bound(rt):
    """rtk_ce_stream_grad_f32 with one output NULL gives the other's bits of the call with both; a max_pos below the
    batch's CSR entries sets bit 3 (value 8) of the error word."""
    lib = rt._lib.load()
    n_ent, B, c, eps = 3003, 70, 100, 0.1
    params, ds, ids, h, r = _case(n_ent, (5, c, c), B, 47, eps, True)
    core, R, S, O = [x.cuda() for x in params]
    flt = rt.DeviceFilter(ds, "cuda")
    slot = flt.slot_of_item[torch.from_numpy(ids).cuda()].contiguous()
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    v, qp = rt.query_vectors(core, R, S, h.cuda(), r.cuda(), packed=True)
    max_pos = B * flt.max_list
    n_entries = int((flt.pair_ptr[slot + 1] - flt.pair_ptr[slot]).sum())
    sp = torch.cuda.current_stream().cuda_stream
    rows = torch.empty(B, dtype=torch.float64, device="cuda")
    lse = torch.empty(B, dtype=torch.float32, device="cuda")
    sc = torch.tensor([3.0 / B], dtype=torch.float32, device="cuda")

    def grad(want_dv, want_go, bound):
        ws = torch.zeros(lib.rtk_ce_stream_workspace_bytes(B, n_ent, c, bound), dtype=torch.uint8, device="cuda")
        rt._lib.check(lib.rtk_ce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, eps, rows.data_ptr(),
                                                 lse.data_ptr(), ws.data_ptr(), ws.numel(), sp), "rows")
        dv = torch.full((B, c), -7.0, device="cuda")
        gO = torch.full((n_ent, c), -7.0, device="cuda")
        rt._lib.check(lib.rtk_ce_stream_grad_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, bound, eps,
                                                 lse.data_ptr(), sc.data_ptr(), dv.data_ptr() if want_dv else None,
                                                 gO.data_ptr() if want_go else None, ws.data_ptr(), ws.numel(), sp), "grad")
        torch.cuda.synchronize()
        return dv, gO, int(ws[:4].view(torch.int32).item())

    dv, gO, err = grad(True, True, max_pos)
    assert err == 0 and not bool((dv == -7.0).all()) and not bool((gO == -7.0).any())
    dv1, gO1, err = grad(True, False, max_pos)
    assert err == 0 and torch.equal(dv1, dv) and bool((gO1 == -7.0).all())
    dv2, gO2, err = grad(False, True, max_pos)
    assert err == 0 and torch.equal(gO2, gO) and bool((dv2 == -7.0).all())
    _, _, err = grad(False, True, n_entries - 1)
    assert err & 8
    _, _, err = grad(False, True, n_entries)
    assert err == 0


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("n_ent,rank,B", [(500, (3, 16, 16), 16), (3003, (5, 100, 100), 70)])
def test_the_op_agrees_with_the_whole_matrix_abi(rt, n_ent, rank, B, eps):
    """ce_loss_1vN(matrix_free=True) is the block loss on the whole range; rtk_ce_stream_rows_f32 / rtk_ce_stream_grad_f32
    share no host code with it.  gO of (loss * 3).backward() has the bits of the ABI's at scale 3 / B: both end in the
    same gradient kernels, which see the forward only through float32(lse).  The loss rows are the same float64 terms
    added in another order (w lse + (lin) against (w lse - t0 sum z) + the positives' part): the float64 row sum moves by
    a few units of 2^-53 relative, so the float32 loss differs from float32(rows.sum() / B) only where that sits on a
    rounding boundary, and then by one float32 ulp.  One query of the batch has an empty list."""
    lib = rt._lib.load()
    c = rank[2]
    params, ds, ids, h, r = _case(n_ent, rank, B, 47, eps, True)
    assert len(ds.objects(int(ids[0]))) == 0
    flt = rt.DeviceFilter(ds, "cuda")
    hc, rc, idc = h.cuda(), r.cuda(), torch.from_numpy(ids).cuda()
    ps = [x.cuda().requires_grad_(True) for x in params]
    loss = rt.ce_loss_1vN(*ps, hc, rc, flt, idc, label_smoothing=eps, matrix_free=True)
    (loss * 3.0).backward()
    O = ps[3].detach()
    slot = flt.slot_of_item[idc].contiguous()
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr(), flt.pair_obj.data_ptr())
    v, qp = rt.query_vectors(*[p.detach() for p in ps[:3]], hc, rc, packed=True)
    max_pos = B * flt.max_list
    sp = torch.cuda.current_stream().cuda_stream
    rows = torch.empty(B, dtype=torch.float64, device="cuda")
    lse = torch.empty(B, dtype=torch.float32, device="cuda")
    sc = torch.tensor([3.0 / B], dtype=torch.float32, device="cuda")
    gO = torch.full((n_ent, c), -7.0, device="cuda")
    ws = torch.zeros(lib.rtk_ce_stream_workspace_bytes(B, n_ent, c, max_pos), dtype=torch.uint8, device="cuda")
    rt._lib.check(lib.rtk_ce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, eps, rows.data_ptr(),
                                             lse.data_ptr(), ws.data_ptr(), ws.numel(), sp), "rows")
    rt._lib.check(lib.rtk_ce_stream_grad_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), n_ent, *csr, max_pos, eps,
                                             lse.data_ptr(), sc.data_ptr(), None, gO.data_ptr(), ws.data_ptr(), ws.numel(),
                                             sp), "grad")
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0
    want = (rows.sum() / B).to(torch.float32)
    near = [torch.nextafter(want, torch.full_like(want, s)) for s in (float("-inf"), float("inf"))]
    print(f"loss {loss.item():.9g}  ABI {want.item():.9g}  its neighbours {near[0].item():.9g} {near[1].item():.9g}; "
          f"gO equal {torch.equal(ps[3].grad, gO)}, max |diff| {(ps[3].grad - gO).abs().max().item():.3e}")
    assert torch.equal(ps[3].grad, gO)
    assert any(torch.equal(loss.detach(), x) for x in [want] + near)


def test_train_py_short_run_with_the_ce_loss(tmp_path, capsys):
    import train
    state = train.main(["--mode", "asymmetric", "--optim", "rsgd", "--seed", "322", "--data",
                        os.path.join(ROOT, "data", "WN18RR") + "/", "--config", "wn18rr_readme", "--epochs", "2",
                        "--max-batches", "12", "--rank", "6", "24", "24", "--checkpoint-path", str(tmp_path),
                        "--set", "train_cfg.loss=ce"])
    out = capsys.readouterr().out
    assert "Final mrr value:" in out and "Final hits@10 value:" in out
    assert len(state.losses.train) == 2 and state.last_epoch == 2
    for hist in (state.losses.train, state.losses.val, state.losses.test, state.losses.norms):
        assert all(math.isfinite(float(x)) for x in hist)
