"""The Riemannian gradient taken at the point (``grad(..., at="point")``, ``grad_at="point"``) through the HIP losses:
the tangent vector against float64 relative to the doubled-rank construct on the matrix form, the ranks that the
construct refuses and the point runs (matrix-free BCE, relation loss), descent, peak memory of a matrix-free ``fit``,
and ``train.py`` with ``train_cfg.grad_at=point train_cfg.matrix_free=true``."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import gen
import relation_grad_model as gm
from oracle import score_oracle as orc
from test_gpu_loss_stream import _batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENT, N_REL, B, EPS, REG = 3003, 7, 70, 0.1, 1e-9
Z_TARGET = 8.0                     # the core is scaled to max |logit| = 8 (asserted < 12: no score saturates)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available()
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _geo(sym):
    from r_tucker_amd.riemannian import SFTuckerRiemannian, TuckerRiemannian
    return SFTuckerRiemannian if sym else TuckerRiemannian


def _components(tv, sym):
    if sym:
        return {"core": tv.delta_core, "R": tv.delta_regular_factors[0], "E": tv.delta_shared_factor}
    return dict(zip(("core", "R", "S", "O"), [tv.delta_core] + list(tv.delta_factors)))


@functools.lru_cache(maxsize=None)
def _case(rank, sym):
    """A point of the manifold in fp32 (factors orthonormalised by a float64 QR, then rounded), a batch with one empty
    query, and the float64 reference: the tangent vector and loss of the construct path on the CPU with a dense torch
    loss on ``oracle.logits_ref``."""
    from r_tucker_amd import driver
    from r_tucker_amd.tucker import SFTucker, Tucker
    core, R, S, O = gen.make_params(N_ENT, N_REL, rank, 61, shared=sym)
    R, S, O = [torch.linalg.qr(torch.from_numpy(f).double())[0].float() for f in (R, S, S if sym else O)]
    ds, ids = _batch(N_ENT, N_REL, B, 61, EPS, empty=True)
    h = torch.from_numpy(ds.features[ids, 0].copy())
    r = torch.from_numpy(ds.features[ids, 1].copy())
    core = torch.from_numpy(core).double()
    core = (core * (Z_TARGET / orc.logits_ref(core, R.double(), S.double(), O.double(), h, r).abs().max().item())).float()
    c64, R64, S64, O64 = [t.double() for t in (core, R, S, O)]
    assert orc.logits_ref(c64, R64, S64, O64, h, r).abs().max().item() < 12.0
    y = ds.dense(ids, torch.float64)

    def dense(T):
        fs = [T.regular_factors[0], T.shared_factor, T.shared_factor] if sym else T.factors
        return F.binary_cross_entropy_with_logits(orc.logits_ref(T.core, *fs, h, r), y)

    x64 = SFTucker(c64, [R64], 2, S64) if sym else Tucker(c64, [R64, S64, O64])
    tv, loss = _geo(sym).grad(driver.RegularisedLoss(dense, REG), x64)
    ref = {k: v.clone() for k, v in _components(tv, sym).items()}
    return {"params": (core, R, S, O), "ds": ds, "ids": ids, "h": h, "r": r, "ref": ref, "ref_loss": loss.item()}


def _model(rt, case, rank, sym):
    core, R, S, O = case["params"]
    model = (rt.SymmetricR_TuckER if sym else rt.AsymmetricR_TuckER)((N_ENT, N_REL), rank)
    with torch.no_grad():
        model.core.copy_(core)
        model.R.weight.copy_(R)
        if sym:
            model.E.weight.copy_(S)
        else:
            model.S.weight.copy_(S)
            model.O.weight.copy_(O)
    return model.cuda()


def _device_batch(rt, case):
    flt = rt.DeviceFilter(case["ds"], "cuda")
    return flt, case["h"].cuda(), case["r"].cuda(), torch.from_numpy(case["ids"]).cuda()


def _errors(tv, sym, ref):
    return {k: (v.double().cpu() - ref[k]).abs().max().item() for k, v in _components(tv, sym).items()}


@functools.lru_cache(maxsize=None)
def _construct_errors(rank, sym):
    """Max-norm errors against float64 of the construct path on the matrix form: the step as it was before ``at``."""
    import r_tucker_amd as rt
    from r_tucker_amd import driver
    case = _case(rank, sym)
    model = _model(rt, case, rank, sym)
    flt, h, r, ids = _device_batch(rt, case)
    tv, loss = _geo(sym).grad(driver.batch_loss_fn(model, h, r, flt, ids, EPS, REG), driver.extract_tensor(model))
    return _errors(tv, sym, case["ref"]), loss.item()


@pytest.mark.parametrize("rank,sym,matrix_free", [((5, 112, 112), False, False), ((5, 112, 112), False, True),
                                                  ((5, 112, 112), True, False), ((5, 112, 112), True, True),
                                                  ((5, 208, 208), False, True)])
def test_tangent_vector_against_float64(rt, rank, sym, matrix_free):
    """Per component: the error of the point path is at most twice the error of the construct path on the matrix form
    (floor 1e-6 max|ref|), the rule of test_gpu_loss_stream.test_accuracy_relative_to_the_matrix_form; the loss within
    2e-6 max(1, |ref|).  The doubled object rank (224, 416) is outside the matrix-free range."""
    from r_tucker_amd import driver
    case = _case(rank, sym)
    ref, ref_loss = case["ref"], case["ref_loss"]
    err_c, loss_c = _construct_errors(rank, sym)
    model = _model(rt, case, rank, sym)
    flt, h, r, ids = _device_batch(rt, case)
    loss_fn = driver.batch_loss_fn(model, h, r, flt, ids, EPS, REG, matrix_free=matrix_free)
    tv, loss = _geo(sym).grad(loss_fn, driver.extract_tensor(model), at="point")
    err_p = _errors(tv, sym, ref)
    print(f"\nrank {rank} {'sym' if sym else 'asym'} {'matrix-free' if matrix_free else 'matrix form'}: "
          f"loss {loss.item():.9g} (construct {loss_c:.9g}, float64 {ref_loss:.9g})")
    for k in ref:
        print(f"  d_{k}: max|ref| {ref[k].abs().max().item():.3e}  err construct {err_c[k]:.3e}  err point {err_p[k]:.3e}")
    assert abs(loss.item() - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss))
    for k in ref:
        assert ref[k].abs().max().item() > 0
        assert err_p[k] <= 2.0 * max(err_c[k], 1e-6 * ref[k].abs().max().item()), k


@pytest.mark.parametrize("sym", [False, True])
def test_what_the_construct_refuses_runs_at_the_point(rt, sym):
    """Manifold rank (5, 112, 112): the construct shows the loss an object rank of 224, which the matrix-free BCE
    (c <= 208) and the relation loss refuse; at the point both see 112."""
    from r_tucker_amd import driver
    rank = (5, 112, 112)
    case = _case(rank, sym)
    model = _model(rt, case, rank, sym)
    flt, h, r, ids = _device_batch(rt, case)
    x = driver.extract_tensor(model)
    geo = _geo(sym)

    def finite(tv, loss):
        assert torch.isfinite(loss)
        for k, v in _components(tv, sym).items():
            assert torch.isfinite(v).all() and v.abs().max().item() > 0, k

    free = driver.batch_loss_fn(model, h, r, flt, ids, EPS, REG, matrix_free=True)
    with pytest.raises(RuntimeError, match="c <= 208"):
        geo.grad(free, x)
    finite(*geo.grad(free, x, at="point"))

    q = gm.grad_case(a=rank[0], b=rank[1], n_rel=N_REL, n_ent=N_ENT, B=B)
    hq, tq, rel = (torch.from_numpy(q[n]).cuda() for n in ("h", "t", "rel"))

    def with_relations(bce):
        def data(T):
            fs = [T.regular_factors[0], T.shared_factor, T.shared_factor] if sym else T.factors
            return bce.data_term(T) + rt.relation_ce_loss(T.core, *fs, hq, tq, rel)
        return driver.RegularisedLoss(data, REG)

    matrix = driver.batch_loss_fn(model, h, r, flt, ids, EPS, REG)
    with pytest.raises(RuntimeError):
        geo.grad(with_relations(matrix), x)                 # the relation term alone: object rank 224 > 208
    tv_b, loss_b = geo.grad(matrix, x, at="point")
    for bce in (matrix, free):
        tv, loss = geo.grad(with_relations(bce), x, at="point")
        finite(tv, loss)
        assert loss.item() > loss_b.item()                  # the relation term is in the loss ...
        assert not torch.equal(tv.delta_core, tv_b.delta_core)          # ... and in the gradient


@pytest.mark.parametrize("mode", ["asymmetric", "symmetric"])
def test_point_gradient_through_the_matrix_free_loss_is_a_descent_direction(mode):
    """The body of test_gpu_driver.test_riemannian_gradient_through_the_hip_loss_is_a_descent_direction with
    at="point" and matrix_free=True."""
    import r_tucker_amd as rt
    from r_tucker_amd import driver
    from r_tucker_amd.data import Data, KG_dataset
    from r_tucker_amd.riemannian import SFTuckerRiemannian, TuckerRiemannian
    torch.manual_seed(5)
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    train_set = KG_dataset(data, data.train_data, label_smoothing=0.1)
    flt = rt.DeviceFilter(train_set, "cuda")
    rank = (6, 24, 24)
    Model = rt.SymmetricR_TuckER if mode == "symmetric" else rt.AsymmetricR_TuckER
    model = Model((len(data.entities), len(data.relations)), rank)
    model.init()
    with torch.no_grad():
        model.core.mul_(2000.0)            # logits of order one: the loss surface has curvature to see
    model.cuda()
    geo = SFTuckerRiemannian if mode == "symmetric" else TuckerRiemannian
    ids = torch.arange(1000, 1512, device="cuda")
    f = flt.features[ids]
    loss_fn = driver.batch_loss_fn(model, f[:, 0].contiguous(), f[:, 1].contiguous(), flt, ids, 0.1, 1e-9, matrix_free=True)
    x = driver.extract_tensor(model)
    rgrad, loss0 = geo.grad(loss_fn, x, at="point")
    gn = rgrad.norm().item()
    assert gn > 0 and torch.isfinite(loss0)
    with torch.no_grad():
        drops = []
        for t in (0.02 * x.norm().item() / gn, 0.005 * x.norm().item() / gn):
            y = (((-t) * rgrad) + geo.TangentVector(rgrad.point)).construct().round(rank)
            drops.append((loss0 - loss_fn(y)).item() / (t * gn * gn))
            for w in ([y.shared_factor] + y.regular_factors if mode == "symmetric" else y.factors):
                w = w.double()
                assert (w.T @ w - torch.eye(w.shape[1], dtype=torch.float64, device=w.device)).abs().max().item() < 5e-5
    # first order: (loss(x) - loss(R(x - t g))) / (t |g|^2) -> 1 as t -> 0
    assert all(0.5 < d < 1.5 for d in drops), drops


def test_fit_allocates_no_batch_times_entities_matrix(rt):
    """N = 400 000, B = 4096 (the score matrix would be 6.5 GB): one ``fit`` of RSGD with ``grad_at="point"`` on the
    matrix-free loss raises the peak by less than B N 4 / 4; what it holds is a small multiple of N c 4 = 51 MB."""
    from r_tucker_amd import driver
    n_ent, n_rel, nb, rank = 400_000, 7, 4096, (4, 32, 32)
    torch.manual_seed(7)
    model = rt.AsymmetricR_TuckER((n_ent, n_rel), rank)
    model.init()
    model.cuda()
    ds, ids = _batch(n_ent, n_rel, nb, 7, EPS, n_pairs=nb)
    flt = rt.DeviceFilter(ds, "cuda")
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    idc = torch.from_numpy(ids).cuda()
    with torch.no_grad():                                   # max |logit| in float64, 256 queries at a time
        c64, R64, S64, O64 = [p.detach().double() for p in (model.core, model.R.weight, model.S.weight, model.O.weight)]
        v = orc.query_vectors_ref(c64, R64, S64, h, r)
        zmax = max((v[lo:lo + 256] @ O64.T).abs().max().item() for lo in range(0, nb, 256))
        model.core.mul_(Z_TARGET / zmax)
        v = orc.query_vectors_ref(model.core.detach().double(), R64, S64, h, r)
        assert max((v[lo:lo + 256] @ O64.T).abs().max().item() for lo in range(0, nb, 256)) < 12.0
        del c64, R64, S64, O64, v
    opt = driver.define_optimizer(model, _cfg(rank, grad_at="point", matrix_free=True, momentum_beta=0.8), "asymmetric", "rsgd")
    assert opt.grad_at == "point"
    loss_fn = driver.batch_loss_fn(model, h, r, flt, idc, EPS, REG, matrix_free=True)
    x_k = driver.extract_tensor(model)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    gn = opt.fit(loss_fn, x_k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"\npeak rise of one fit {rise / 1e6:.1f} MB; the matrix is {nb * n_ent * 4 / 1e6:.0f} MB, N c 4 = {n_ent * rank[2] * 4 / 1e6:.0f} MB")
    assert torch.isfinite(gn) and gn.item() > 0 and torch.isfinite(opt.loss)
    assert rise < nb * n_ent * 4 // 4


def _cfg(rank, **train):
    from configs.base_config import Config
    cfg = Config(None)
    cfg.model_cfg.manifold_rank = rank
    for k, v in train.items():
        setattr(cfg.train_cfg, k, v)
    return cfg


@pytest.mark.parametrize("mode,optim,loss", [("asymmetric", "rsgd", "bce"), ("symmetric", "adam", "bce"),
                                             ("asymmetric", "rgd", "ce")])
def test_train_py_short_run_at_the_point_matrix_free(tmp_path, capsys, mode, optim, loss):
    """Manifold rank (6, 112, 112): with the defaults the step scores at object rank 224 on the matrix form; here it
    runs at 112 without the matrix."""
    import train
    state = train.main(["--mode", mode, "--optim", optim, "--seed", "322", "--data", os.path.join(ROOT, "data", "WN18RR") + "/",
                        "--config", "wn18rr_readme", "--epochs", "2", "--max-batches", "3", "--rank", "6", "112", "112",
                        "--checkpoint-path", str(tmp_path), "--set", f"train_cfg.loss={loss}",
                        "--set", "train_cfg.grad_at=point", "--set", "train_cfg.matrix_free=true"])
    assert "Final mrr value:" in capsys.readouterr().out
    assert len(state.losses.train) == 2 and state.last_epoch == 2
    for hist in (state.losses.train, state.losses.val, state.losses.test, state.losses.norms):
        assert all(math.isfinite(float(x)) for x in hist)
    for k, w in state.model.items():
        if k.endswith(".weight"):
            w = w.detach().double()
            assert (w.T @ w - torch.eye(w.shape[1], dtype=torch.float64, device=w.device)).abs().max().item() < 5e-5, k
    assert set(state.model.keys()) == ({"core", "E.weight", "R.weight"} if mode == "symmetric"
                                       else {"core", "S.weight", "R.weight", "O.weight"})
