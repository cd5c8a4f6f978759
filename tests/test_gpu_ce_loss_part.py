"""The softmax cross-entropy loss on blocks of entity rows (ce_partials_block_1vN, ce_merge_lse, ce_loss_block_1vN and
ShardedEntityScorer.ce_loss_1vN over rtk_ce_stream_*_part_f32) end to end: three blocks emulated on one GPU with
``lse=`` against float64 (ce_cases.ce_ref) at the bounds of test_gpu_ce_loss.py -- loss <= 2e-6 max(1, |ref|), each
gradient <= 2e-4 max|ref| + 1e-9 in the max norm, the loss times 3.0 before backward() --, large logits, world size 1,
peak memory, determinism and two real ranks."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                       # a rank of test_two_real_ranks: a fresh process, no conftest
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]

import ce_cases  # noqa: E402
import gen  # noqa: E402
from oracle import score_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _emulate(rt, leaves, O_leaf, cuts, n_ent, h, r, flt, idc, eps, backward=True):
    """P ranks on one GPU: every block's forward state, the merged lse, then every block's share with ``lse=``; O_loc is
    a slice of the leaf.  -> (the loss as the float64 sum of the shares, the shares, lse)."""
    blocks = list(zip(cuts[:-1], cuts[1:]))
    parts = [rt.ce_partials_block_1vN(*leaves, O_leaf[a:b], a, n_ent, h, r, flt, idc, label_smoothing=eps) for a, b in blocks]
    lse = rt.ce_merge_lse([p[0] for p in parts], [p[1] for p in parts])
    shares = []
    for a, b in blocks:
        share = rt.ce_loss_block_1vN(*leaves, O_leaf[a:b], a, n_ent, h, r, flt, idc, label_smoothing=eps, lse=lse)
        if backward:
            (share * 3.0).backward()                           # a non-unit upstream gradient
        shares.append(share.detach())
    return sum(s.double().item() for s in shares), shares, lse


def _check(rt, n_ent, rank, B, eps, cuts, empty, shared=False, seed=41, core_scale=1.0, loss_tol=None, grad_rel=2e-4):
    params, ds, ids, h, r = _case(n_ent, rank, B, seed, eps, empty, core_scale, shared)
    ref = ce_cases.ce_ref(*params, h, r, ds.targets(ids, eps), shared=shared)
    flt = rt.DeviceFilter(ds, "cuda")
    dc, dR, dS = [x.clone().cuda().requires_grad_(True) for x in params[:3]]
    dO = dS if shared else params[3].clone().cuda().requires_grad_(True)
    if empty and eps == 0.0:                                   # the empty-list query: a row of mass w_d = 0
        assert len(ds.objects(int(ids[0]))) == 0
    loss, _, _ = _emulate(rt, (dc, dR, dS), dO, cuts, n_ent, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(), eps)
    got = [dc.grad, dR.grad, dS.grad] + ([] if shared else [dO.grad])
    tol = 2e-6 * max(1.0, abs(ref[0].item())) if loss_tol is None else loss_tol
    print(f"loss {loss:.9g} ref {ref[0].item():.9g} (bound {tol:.3e}); max|z| {ref[-1]:.3f}")
    assert math.isfinite(loss)
    assert abs(loss - ref[0].item()) <= tol
    assert len(got) == len(ref) - 2
    for g, e in zip(got, ref[1:-1]):
        e = 3.0 * e
        assert g.shape == e.shape
        err = (g.double().cpu() - e).abs().max().item()
        print(f"grad {tuple(e.shape)}: err {err:.3e} of max {e.abs().max().item():.3e}")
        assert err <= grad_rel * e.abs().max().item() + 1e-9


@pytest.mark.parametrize("mode", ["asym", "sym"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_three_blocks_against_float64(rt, mode, eps):
    _check(rt, 3001, (5, 32, 32), 48, eps, [0, 1000, 1999, 3001], True, shared=(mode == "sym"))


def test_large_logits(rt):
    """The core scale of test_gpu_ce_loss.py::test_large_logits (max |z| near 100) over two blocks, at that test's bound."""
    n_ent, rank, B, eps, seed = 3003, (5, 64, 64), 33, 0.1, 41
    params, ds, ids, h, r = _case(n_ent, rank, B, seed, eps, True)
    z1 = orc.logits_ref(*[p.double() for p in params], h, r).abs().max().item()
    scale = 100.0 / z1
    params, ds, ids, h, r = _case(n_ent, rank, B, seed, eps, True, core_scale=scale)
    zmax = orc.logits_ref(*[p.double() for p in params], h, r).abs().max().item()
    assert 50.0 <= zmax <= 200.0
    pz = 2 * 2e-5 * (1.0 + zmax)
    _check(rt, n_ent, rank, B, eps, [0, 1501, 3003], True, core_scale=scale, loss_tol=pz, grad_rel=2e-4 + pz)


def test_mode_checks_on_the_device(rt):
    params, ds, ids, h, r = _case(500, (3, 16, 16), 16, 3, 0.1, False)
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [x.cuda() for x in params]
    hc, rc, idc = h.cuda(), r.cuda(), torch.from_numpy(ids).cuda()
    with pytest.raises(ValueError, match="not the loss"):
        rt.ce_loss_block_1vN(*ps[:3], ps[3][100:200], 100, 500, hc, rc, flt, idc)
    with pytest.raises(RuntimeError, match="is not a part of"):
        rt.ce_loss_block_1vN(*ps[:3], ps[3][100:200], 450, 500, hc, rc, flt, idc,
                             lse=torch.zeros(16, dtype=torch.float64, device="cuda"))
    # the whole range needs neither lse nor collectives and is the loss: ce_loss_1vN(matrix_free=True) is this call
    runs = []
    for block in (True, False):
        leaves = [p.clone().requires_grad_(True) for p in ps]
        if block:
            loss = rt.ce_loss_block_1vN(*leaves, 0, 500, hc, rc, flt, idc, label_smoothing=0.1)
        else:
            loss = rt.ce_loss_1vN(*leaves, hc, rc, flt, idc, label_smoothing=0.1, matrix_free=True)
        (loss * 3.0).backward()
        runs.append([loss.detach()] + [p.grad for p in leaves])
    assert len(runs[0]) == 5
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # batch == 0: a zero loss and zero gradients; an empty block: a zero share, an empty gradient
    leaves = [p.clone().requires_grad_(True) for p in ps[:3]]
    O_blk = ps[3][100:200].clone().requires_grad_(True)
    loss = rt.ce_loss_block_1vN(*leaves, O_blk, 100, 500, hc[:0], rc[:0], flt, idc[:0], label_smoothing=0.1,
                                lse=torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert loss.dtype == torch.float32 and loss.item() == 0.0
    loss.backward()
    assert all(p.grad is not None and not p.grad.any() for p in leaves + [O_blk])
    O_none = ps[3][:0].clone().requires_grad_(True)
    m, s, lin = rt.ce_partials_block_1vN(*ps[:3], O_none, 500, 500, hc, rc, flt, idc)
    assert bool(torch.isinf(m).all()) and not s.any() and not lin.any()
    share = rt.ce_loss_block_1vN(*leaves, O_none, 500, 500, hc, rc, flt, idc, label_smoothing=0.1,
                                 lse=torch.zeros(16, dtype=torch.float64, device="cuda"))
    share.backward()
    assert share.item() == 0.0 and O_none.grad.shape == (0, 16)


def test_world_size_one_is_the_matrix_free_loss(rt):
    """ShardedEntityScorer.ce_loss_1vN without a process group: the bits of ce_loss_1vN(matrix_free=True)."""
    n_ent, eps = 3001, 0.1
    params, ds, ids, h, r = _case(n_ent, (5, 32, 32), 48, 41, eps, True)
    flt = rt.DeviceFilter(ds, "cuda")
    hc, rc, idc = h.cuda(), r.cuda(), torch.from_numpy(ids).cuda()
    runs = []
    for sharded in (False, True):
        ps = [x.clone().cuda().requires_grad_(True) for x in params]
        if sharded:
            loss = rt.ShardedEntityScorer(n_ent).ce_loss_1vN(*ps, hc, rc, flt, idc, label_smoothing=eps)
        else:
            loss = rt.ce_loss_1vN(*ps, hc, rc, flt, idc, label_smoothing=eps, matrix_free=True)
        (loss * 3.0).backward()
        runs.append([loss.detach()] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_batch_times_block_allocation(rt):
    """Rows [300 000, 400 000) of n_ent = 400 000 at B = 2048 (the logit block would be 819 MB): the forward states of
    all four blocks, the merge, and the forward and backward of the last block raise the peak by less than
    B n_local 4 / 8 bytes.  S has 1000 rows (its dense gradient is not what is measured)."""
    n_ent, n_loc, n_rel, B, rank, eps = 400_000, 100_000, 7, 2048, (4, 64, 64), 0.1
    core, R, S, _ = gen.make_params(1000, n_rel, rank, 5)
    O = gen.make_params(n_ent, n_rel, rank, 5)[3]
    core = (core * 0.4).astype(np.float32)
    ds, ids = ce_cases.batch(n_ent, n_rel, B, 5, eps, n_pairs=B)
    flt = rt.DeviceFilter(ds, "cuda")
    leaves = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (core, R, S)]
    O_all = torch.from_numpy(O).cuda()
    O_blk = O_all[300_000:].clone().requires_grad_(True)
    h = torch.from_numpy(ds.features[ids, 0].copy() % 1000).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    parts = [rt.ce_partials_block_1vN(*leaves, O_all[a:a + n_loc], a, n_ent, h, r, flt, idc, label_smoothing=eps)
             for a in range(0, n_ent, n_loc)]
    lse = rt.ce_merge_lse([p[0] for p in parts], [p[1] for p in parts])
    share = rt.ce_loss_block_1vN(*leaves, O_blk, 300_000, n_ent, h, r, flt, idc, label_smoothing=eps, lse=lse)
    (share * 3.0).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.1f} MB; the logit block is {B * n_loc * 4 / 1e6:.0f} MB")
    assert rise < B * n_loc * 4 // 8
    assert math.isfinite(share.item()) and bool(torch.isfinite(O_blk.grad).all()) and bool(O_blk.grad.any())
    # the blocks' softmass masses sum to one: the merged lse is the whole row's
    sigma = sum(p[1] * torch.exp(p[0].double() - lse) for p in parts)
    assert (sigma - 1.0).abs().max().item() <= 1e-12


def test_determinism_and_no_grad(rt):
    n_ent, eps, cuts = 3003, 0.1, [0, 1001, 2002, 3003]
    params, ds, ids, h, r = _case(n_ent, (5, 100, 100), 70, 47, eps, True)
    flt = rt.DeviceFilter(ds, "cuda")
    hc, rc, idc = h.cuda(), r.cuda(), torch.from_numpy(ids).cuda()
    runs = []
    for _ in range(2):
        ps = [x.clone().cuda().requires_grad_(True) for x in params]
        _, shares, lse = _emulate(rt, ps[:3], ps[3], cuts, n_ent, hc, rc, flt, idc, eps)
        runs.append(shares + [lse] + [p.grad for p in ps])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with torch.no_grad():
        _, quiet, _ = _emulate(rt, ps[:3], ps[3], cuts, n_ent, hc, rc, flt, idc, eps, backward=False)
    for a, b in zip(quiet, runs[0][:3]):
        assert not a.requires_grad and torch.equal(a, b)


# ---- two real ranks ------------------------------------------------------------------------------------------------

def _two_rank_case():
    n_ent, B, eps = 3001, 48, 0.1                          # odd: the last shard has a padding row
    return (n_ent, eps) + tuple(_case(n_ent, (5, 32, 32), B, 41, eps, True))


def _rank_main(rank, port, out_path):
    """One rank of world size 2 over RCCL: loss and gradients of ShardedEntityScorer.ce_loss_1vN into an .npz."""
    import torch.distributed as dist
    import r_tucker_amd as rt
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=2)
    try:
        n_ent, eps, params, ds, ids, h, r = _two_rank_case()
        flt = rt.DeviceFilter(ds, "cuda")
        sc = rt.ShardedEntityScorer(n_ent)
        dev = [x.cuda() for x in params]
        ps = [x.clone().requires_grad_(True) for x in dev[:3]] + [sc.local_block(dev[3]).requires_grad_(True)]
        loss = sc.ce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(), label_smoothing=eps)
        (loss * 3.0).backward()
        torch.cuda.synchronize()
        np.savez(out_path, loss=loss.item(), **{f"g{i}": p.grad.cpu().numpy() for i, p in enumerate(ps)})
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_real_ranks(rt, tmp_path):
    """World size 2 over RCCL (each rank a fresh child process under its own time limit) equals the world-size-1 result
    within the end-to-end bounds; the gradients of core, R and S are equal on the two ranks."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"          # dmabuf IPC (RCCL across processes)
    outs = [str(tmp_path / f"rank{k}.npz") for k in range(2)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--rank", str(k),
                               str(port), outs[k]], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for k in range(2)]
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
    n_ent, eps, params, ds, ids, h, r = _two_rank_case()
    flt = rt.DeviceFilter(ds, "cuda")
    ps = [x.clone().cuda().requires_grad_(True) for x in params]
    loss = rt.ShardedEntityScorer(n_ent).ce_loss_1vN(*ps, h.cuda(), r.cuda(), flt, torch.from_numpy(ids).cuda(),
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
