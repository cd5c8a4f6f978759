"""The Riemannian optimizer steps on a row-sharded object factor (``ShardedEntityScorer.tucker`` / ``.row_sum``,
``Tucker(row_sum=...)``) under the gloo backend, world size 2, on the CPU in float64.

Every rank holds its block of O (the last one padded with a zero row: n_ent is odd) and the replicated core, R and S,
and takes three steps of each optimizer at both ``grad_at`` forms on ``sc.tucker(...)``, with
``sc.bce_loss_1vN`` as the loss (its block steps injected as float64 CPU functions, as in test_sharded_loss_gloo.py).
The parent takes the same steps on the whole factors with the oracle's loss.  The two differ only in where the sums
over O's rows are cut, so every parameter must agree to float64 round-off: 1e-10 of its max-norm (the block-sum
emulation measured 5e-15; a real difference of method shows at 3e-8 after one step).  S has its own row count: with
``S.shape == O.shape`` the unsharded retraction batches the two factors (plain HOSVD among them), a sharded one never
does, and the two orders differ by 3e-8."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import score_oracle as orc
from test_sharded_loss_gloo import EPS, _case, _cpu_grad_o, _cpu_rows, _cpu_stage1_bwd, _free_port

N_ENT = 101                      # odd: rank 1's block ends in a padding row
N_SUBJ = 37
STEPS = 3
OPTIMIZERS = ("RGD", "RSGDwithMomentum", "RiemannianAdam")
GRAD_AT = ("construct", "point")
LR = 0.05


def _point():
    """An orthonormal point (float64) and the loss data of ``_case``."""
    core, R, S, O, _, r, flt, y = _case(N_ENT)
    S = S[:N_SUBJ]                                                # its own row count (the module docstring's trap)
    h = torch.arange(r.numel()) * 7 % N_SUBJ
    R, S, O = [torch.linalg.qr(f)[0].contiguous() for f in (R, S, O)]
    assert S.shape[0] != O.shape[0] and S.shape[0] != -(-N_ENT // 2)
    return core, R, S, O, h, r, flt, y


def _make(name, params, rank3, grad_at):
    from r_tucker_amd.model.asymmetric import optim
    return getattr(optim, name)(params, rank3, LR, grad_at=grad_at)


def _run(name, grad_at, core, R, S, O, make_point, loss_fn):
    """STEPS steps on clones of the parameters (order ``[core, S, R, O]``); returns them."""
    core, R, S, O = [torch.nn.Parameter(t.clone()) for t in (core, R, S, O)]
    opt = _make(name, [core, S, R, O], tuple(core.shape), grad_at)
    for _ in range(STEPS):
        x_k = make_point(core.data, R.data, S.data, O.data)
        opt.fit(loss_fn, x_k)
        opt.step()
    return [t.data.clone() for t in (core, R, S, O)]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _worker_body(rank)))
    except BaseException as e:                                    # the parent fails at once instead of waiting
        import traceback
        q.put((rank, traceback.format_exc() or repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def _worker_body(rank):
    """One rank: the three steps of every optimizer and form on its block, and what the all-reduces carried."""
    from r_tucker_amd.sharded import ShardedEntityScorer
    core, R, S, O, h, r, flt, _ = _point()
    B = h.numel()
    reduced = []
    real_all_reduce = dist.all_reduce

    def recording_all_reduce(t, *a, **kw):
        reduced.append(tuple(t.shape))
        return real_all_reduce(t, *a, **kw)
    dist.all_reduce = recording_all_reduce

    sc = ShardedEntityScorer(N_ENT, query_vectors_fn=lambda c_, R_, S_, hh, rr, **kw: orc.query_vectors_ref(
        c_.detach(), R_.detach(), S_.detach(), hh, rr))
    sc.pack_fn = lambda v, dtype: v
    lo, hi = sc.shards.bounds(rank)

    def loss_fn(T):
        return sc.bce_loss_1vN(T.core, T.factors[0], T.factors[1], T.factors[2], h, r, flt, torch.arange(B),
                               label_smoothing=EPS, rows_fn=_cpu_rows, grad_o_fn=_cpu_grad_o,
                               stage1_bwd_fn=_cpu_stage1_bwd)

    out = {}
    for name in OPTIMIZERS:
        for at in GRAD_AT:
            del reduced[:]
            c1, R1, S1, O1 = _run(name, at, core, R, S, sc.local_block(O), sc.tucker, loss_fn)
            # what the loss itself reduces: the B loss rows and dv (B x c, or B x 2c on the construct); everything
            # else went through row_sum and must be a small square-ish matrix or a scalar, never anything with rows
            widths = {core.shape[2], 2 * core.shape[2]}
            loss_shapes = {(B,)} | {(B, w) for w in widths}
            step_shapes = [s for s in reduced if s not in loss_shapes]
            small = all(len(s) in (0, 2) and all(d in widths for d in s) for s in step_shapes)
            out[(name, at)] = (c1.numpy(), R1.numpy(), S1.numpy(), O1[: hi - lo].numpy(),
                               bool(small and step_shapes), not bool(O1[hi - lo:].any()), O1.shape[0] - (hi - lo))
    # Tucker.norm() under autograd (the regulariser inside a differentiated loss_fn) and both tangent norms
    from r_tucker_amd import riemannian as rm
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, sc.local_block(O))]
    T = sc.tucker(*leaves)
    val = T.norm() ** 2
    val.backward()
    tv = rm.TuckerTangentVector(sc.tucker(core, R, S, sc.local_block(O)), 0.5 * core,
                                [0.1 * R, 0.2 * S, 0.3 * sc.local_block(O)])
    norms = []
    for kind in ("frobenius", "coordinate"):
        rm.EXPERIMENT["norm"] = kind
        norms.append(float(tv.norm()))
    rm.EXPERIMENT["norm"] = "frobenius"
    out["norm"] = (val.item(), leaves[0].grad.numpy(), leaves[3].grad[: hi - lo].numpy(), norms)
    return out


@pytest.fixture(scope="module")
def sharded_runs():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(rk, 2, port, q)) for rk in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(120)
    assert all(isinstance(r[1], dict) for r in res), [r[1] for r in res if not isinstance(r[1], dict)]
    assert all(p.exitcode == 0 for p in procs)
    return [r[1] for r in res]


@pytest.fixture(scope="module")
def point():
    return _point()


@pytest.mark.parametrize("grad_at", GRAD_AT)
@pytest.mark.parametrize("name", OPTIMIZERS)
def test_sharded_steps_equal_unsharded_world2_gloo(sharded_runs, point, name, grad_at):
    import numpy as np
    from r_tucker_amd.tucker import Tucker
    core, R, S, O, h, r, _, y = point

    def loss_fn(T):
        return orc.bce_mean_ref(orc.score_ref(T.core, T.factors[0], T.factors[1], T.factors[2], h, r), y)

    want = _run(name, grad_at, core, R, S, O, lambda c_, R_, S_, O_: Tucker(c_, [R_, S_, O_]), loss_fn)
    moved = max(float((w - p0).abs().max()) for w, p0 in zip(want, (core, R, S, O)))
    assert moved > 1e-4                                           # the steps did something
    r0, r1 = sharded_runs[0][(name, grad_at)], sharded_runs[1][(name, grad_at)]
    for a, b in zip(r0[:3], r1[:3]):                              # core, R, S: the same bits on both ranks
        assert np.array_equal(a, b)
    got = list(r0[:3]) + [np.concatenate([r0[3], r1[3]], axis=0)]
    for nm, g, w in zip(("core", "R", "S", "O"), got, want):
        w = w.numpy()
        err, scale = np.abs(g - w).max(), np.abs(w).max()
        print(f"{name} {grad_at} {nm}: max-norm distance {err:.3e} of {scale:.3e}")
        assert g.shape == w.shape and err <= 1e-10 * scale
    for res in (r0, r1):
        assert res[4], "something other than a small matrix went through all_reduce"
        assert res[5], "a padding row moved"
    assert r0[6] == 0 and r1[6] == 1                              # rank 1 holds the one padding row


def test_norms_sum_over_the_shards_and_differentiate(sharded_runs, point):
    """``Tucker.norm()`` inside autograd: forward sums over the ranks, backward passes the complete matrix's gradient
    through, so the core's gradient is whole on every rank and O's is this rank's rows; both tangent norms too."""
    import numpy as np
    from r_tucker_amd import riemannian as rm
    from r_tucker_amd.tucker import Tucker
    core, R, S, O = point[:4]
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
    val = Tucker(leaves[0], leaves[1:]).norm() ** 2
    val.backward()
    tv = rm.TuckerTangentVector(Tucker(core, [R, S, O]), 0.5 * core, [0.1 * R, 0.2 * S, 0.3 * O])
    want = []
    try:
        for kind in ("frobenius", "coordinate"):
            rm.EXPERIMENT["norm"] = kind
            want.append(float(tv.norm()))
    finally:
        rm.EXPERIMENT["norm"] = "frobenius"
    n0, n1 = sharded_runs[0]["norm"], sharded_runs[1]["norm"]
    for n in (n0, n1):
        assert abs(n[0] - val.item()) <= 1e-12 * val.item()
        assert np.abs(n[1] - leaves[0].grad.numpy()).max() <= 1e-12 * float(leaves[0].grad.abs().max())
        assert np.allclose(n[3], want, rtol=1e-12, atol=0)
    gO = np.concatenate([n0[2], n1[2]], axis=0)
    assert np.abs(gO - leaves[3].grad.numpy()).max() <= 1e-12 * float(leaves[3].grad.abs().max())
    assert abs(want[0] - want[1]) > 1e-3 * want[0]              # the two norms are different numbers
