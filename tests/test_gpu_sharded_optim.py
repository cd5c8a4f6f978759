"""Three Riemannian steps on ``ShardedEntityScorer.tucker(...)`` on the device, one process (world size 1: ``row_sum`` is
the identity callable, but every product that sums over O's rows takes the sharded path, and the float64 Gram matrices
of the retraction come from ``rtk_tall_gram_f64``).

Yardstick: the same three steps in float64 on the CPU, the loss restated in torch (the oracle's BCE on the dense
smoothed targets).  Bound: for each parameter the max-norm distance of the sharded fp32 run to that trajectory is at
most TWICE the distance of the unsharded fp32 run (``Tucker`` without ``row_sum``, the same loss on the same device).
The two fp32 runs differ only in the order of sums that are exact or float64 -- the Gram matrices behind the Cholesky
factors -- so they sit at the same distance up to the fp32 roundings that follow; the factor 2 covers those."""
import numpy as np
import pytest
import torch

from gen import make_params
from oracle import score_oracle as orc
from test_gpu_loss_stream_bf16 import _Pairs

pytestmark = pytest.mark.gpu

RANK, N_ENT, N_SUBJ, N_REL, B, EPS, STEPS, LR = (3, 32, 32), 3003, 2000, 7, 70, 0.1, 3, 0.05
ORTH_TOL = 5e-5          # tests/test_gpu_driver.py: orthonormality of a retracted fp32 factor


def _case():
    core, R, S, O = [torch.from_numpy(x).double() for x in make_params(N_ENT, N_REL, RANK, 61)]
    R, S, O = [torch.linalg.qr(f)[0].contiguous() for f in (R, S[:N_SUBJ], O)]
    rng = np.random.default_rng(61)
    pairs = [(int(s), int(r_)) for s, r_ in zip(rng.permutation(N_SUBJ)[:B], rng.integers(0, N_REL, B))]
    lists = [np.unique(rng.integers(0, N_ENT, int(rng.integers(1, 9)))).tolist() for _ in pairs]
    ds = _Pairs(pairs, lists, N_ENT, EPS)
    ids = np.arange(B, dtype=np.int64)
    h, r = torch.from_numpy(ds.features[ids, 0].copy()), torch.from_numpy(ds.features[ids, 1].copy())
    y = torch.full((B, N_ENT), EPS / N_ENT, dtype=torch.float64)
    for d, l in enumerate(lists):
        y[d, l] += 1.0 - EPS
    return (core, R, S, O), ds, h, r, torch.from_numpy(ids), y


def _steps(params, make_point, loss_fn):
    from r_tucker_amd.model.asymmetric.optim import RSGDwithMomentum
    core, R, S, O = [torch.nn.Parameter(t.clone()) for t in params]
    opt = RSGDwithMomentum([core, S, R, O], RANK, LR, grad_at="point")
    for _ in range(STEPS):
        opt.fit(loss_fn, make_point(core.data, R.data, S.data, O.data))
        opt.step()
    return [t.data.double().cpu() for t in (core, R, S, O)]


def test_sharded_steps_track_float64_like_unsharded_ones():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd as rt
    from r_tucker_amd import smalllinalg as sl
    from r_tucker_amd.tucker import Tucker
    params, ds, h, r, ids, y = _case()
    want = _steps(params, lambda c_, R_, S_, O_: Tucker(c_, [R_, S_, O_]),
                  lambda T: orc.bce_mean_ref(orc.score_ref(T.core, *T.factors, h, r), y))
    assert max(float((w - p0).abs().max()) for w, p0 in zip(want, params)) > 1e-4       # the steps moved the point

    flt = rt.DeviceFilter(ds, "cuda")
    sc = rt.ShardedEntityScorer(N_ENT)
    assert sc.world == 1 and sc.row_sum is not None
    hd, rd, idd = h.cuda(), r.cuda(), ids.cuda()
    dev = [t.float().cuda() for t in params]

    def loss_fn(T):
        return sc.bce_loss_1vN(T.core, *T.factors, hd, rd, flt, idd, label_smoothing=EPS)

    calls = []
    kernel = sl.tall_gram_f64_rows
    sl.tall_gram_f64_rows = lambda A, Bm: (calls.append(tuple(A.shape)), kernel(A, Bm))[1]
    try:
        plain = _steps(dev, lambda c_, R_, S_, O_: Tucker(c_, [R_, S_, O_]), loss_fn)
        assert not calls                                      # row_sum=None: today's path, the kernel is not involved
        shard = _steps(dev, sc.tucker, loss_fn)
    finally:
        sl.tall_gram_f64_rows = kernel
    assert calls == [(N_ENT, RANK[2])] * (2 * STEPS)          # two Cholesky-QR rounds of O's new block per step

    for name, w, a, b in zip(("core", "R", "S", "O"), want, plain, shard):
        d_plain, d_shard = float((a - w).abs().max()), float((b - w).abs().max())
        print(f"{name}: distance to the float64 trajectory {d_shard:.3e} sharded, {d_plain:.3e} unsharded "
              f"(max-norm {float(w.abs().max()):.3e})")
        assert np.isfinite(d_shard) and d_shard <= 2.0 * d_plain, name
    for f in shard[1:]:
        gram = f.T @ f
        assert float((gram - torch.eye(gram.shape[0], dtype=gram.dtype)).abs().max()) < ORTH_TOL
