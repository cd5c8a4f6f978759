"""The Riemannian gradient taken at the point (``grad(..., at="point")``) on the CPU in float64: the same tangent
vector and loss as the doubled-rank construct, the rank that ``loss_fn`` sees, the unchanged default, the optimizers'
``grad_at`` keyword, and the ``train_cfg.grad_at`` / ``train_cfg.matrix_free`` switches with their refusals."""
import os
import types

import pytest
import torch
import torch.nn.functional as F

from test_riemannian import DT, deltas, geo, point

from r_tucker_amd import driver
from r_tucker_amd.tucker import SFTucker, Tucker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["RGD", "RSGDwithMomentum", "RiemannianAdam"]


def _bce(x, seed=9):
    """A dense BCE-with-logits on ``T.full()`` against fixed targets in [0, 1]: a function of the represented tensor."""
    y = torch.rand(x.full().shape, dtype=DT, generator=torch.Generator().manual_seed(seed))
    return lambda T: F.binary_cross_entropy_with_logits(T.full(), y)


def _components(tv, sym):
    return [tv.delta_core] + list(deltas(tv, sym))


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("regularised", [False, True])
def test_point_and_construct_give_the_same_tangent_vector(sym, regularised):
    x = point(sym)
    loss_fn = _bce(x)
    if regularised:
        loss_fn = driver.RegularisedLoss(loss_fn, 0.37)
    want, loss_c = geo(sym).grad(loss_fn, x)
    got, loss_p = geo(sym).grad(loss_fn, x, at="point")
    for a, b in zip(_components(got, sym), _components(want, sym)):
        assert a.shape == b.shape
        assert b.abs().max().item() > 0
        assert torch.allclose(a, b, rtol=0.0, atol=1e-10)
    assert abs(loss_p.item() - loss_c.item()) <= 1e-10 * abs(loss_c.item())
    assert abs(got.norm().item() - want.norm().item()) <= 1e-10
    # an undeclared regulariser (no riemannian_split) is differentiated through the container's norm in both forms
    if regularised:
        plain = lambda T: loss_fn.data_term(T) + 0.37 * T.norm() ** 2      # noqa: E731
        auto, loss_a = geo(sym).grad(plain, x, at="point")
        for a, b in zip(_components(auto, sym), _components(want, sym)):
            assert torch.allclose(a, b, rtol=0.0, atol=1e-10)
        assert abs(loss_a.item() - loss_c.item()) <= 1e-10 * abs(loss_c.item())


@pytest.mark.parametrize("sym", [False, True])
def test_rank_seen_by_the_loss(sym):
    x = point(sym)
    rank = tuple(x.core.shape)
    inner, seen = _bce(x), []

    def loss_fn(T):
        widths = [f.shape[1] for f in (T.regular_factors + [T.shared_factor] if sym else T.factors)]
        seen.append((tuple(T.core.shape), widths))
        return inner(T)

    own = [rank[0], rank[1]] if sym else list(rank)
    geo(sym).grad(loss_fn, x, at="point")
    assert seen == [(rank, own)]
    del seen[:]
    geo(sym).grad(loss_fn, x)
    assert seen == [(tuple(2 * r for r in rank), [2 * w for w in own])]
    # through an optimizer built with grad_at="point"
    del seen[:]
    model, params, extract, mod = _model(sym, (7, 11, 11), rank)
    opt = mod.RGD(params, rank, 0.1, grad_at="point")
    opt.fit(loss_fn, extract())
    assert seen == [(rank, own)]


@pytest.mark.parametrize("sym", [False, True])
def test_default_is_the_construct_and_a_bad_value_is_refused(sym):
    x = point(sym)
    loss_fn = driver.RegularisedLoss(_bce(x), 0.37)
    a, loss_a = geo(sym).grad(loss_fn, x)
    b, loss_b = geo(sym).grad(loss_fn, x, at="construct")
    for p, q in zip(_components(a, sym), _components(b, sym)):
        assert torch.equal(p, q)
    assert torch.equal(loss_a, loss_b)
    for bad in ("bogus", "Point", None):
        with pytest.raises(ValueError, match="construct, point"):
            geo(sym).grad(loss_fn, x, at=bad)
    # the leaves of the point form stand for the point: it is left without a gradient and without requires_grad
    geo(sym).grad(loss_fn, x, at="point")
    assert not x.core.requires_grad and x.core.grad is None


def _model(sym, shape, rank, seed=3, core_scale=3.0):
    """The model, parameter list and ``extract`` of test_optimizers_descend_and_keep_the_manifold."""
    import r_tucker_amd as rt
    mod = __import__("r_tucker_amd.model.%s.optim" % ("symmetric" if sym else "asymmetric"), fromlist=["x"])
    Model = rt.SymmetricR_TuckER if sym else rt.AsymmetricR_TuckER
    torch.manual_seed(seed)
    model = Model((shape[1], shape[0]), rank).double()
    model.init()
    with torch.no_grad():
        model.core.mul_(core_scale)
    if sym:
        params = torch.nn.ParameterList([model.core, model.E.weight, model.R.weight])
        extract = lambda: SFTucker(model.core.data, [model.R.weight], num_shared_factors=2, shared_factor=model.E.weight)  # noqa: E731
    else:
        params = torch.nn.ParameterList([model.core, model.S.weight, model.R.weight, model.O.weight])
        extract = lambda: Tucker(model.core.data, [model.R.weight, model.S.weight, model.O.weight])  # noqa: E731
    return model, params, extract, mod


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("opt_name", OPTS)
def test_optimizer_direction_after_one_fit(sym, opt_name):
    shape, rank = (6, 9, 9), (2, 3, 3)
    got = {}
    for at in ("construct", "point"):
        model, params, extract, mod = _model(sym, shape, rank)
        x_k = extract()
        opt = getattr(mod, opt_name)(params, rank, 0.3, grad_at=at)
        assert opt.grad_at == at
        gn = opt.fit(driver.RegularisedLoss(_bce(x_k), 0.37), x_k, normalize_grad=False if opt_name != "RiemannianAdam" else 1.0)
        got[at] = (_components(opt.direction, sym), gn, opt.loss)
    for a, b in zip(got["point"][0], got["construct"][0]):
        assert b.abs().max().item() > 0
        assert torch.allclose(a, b, rtol=0.0, atol=1e-10)
    assert abs(got["point"][1].item() - got["construct"][1].item()) <= 1e-10
    assert abs(got["point"][2].item() - got["construct"][2].item()) <= 1e-10 * abs(got["construct"][2].item())
    default = getattr(mod, opt_name)(_model(sym, shape, rank)[1], rank, 0.3)
    assert default.grad_at == "construct"
    with pytest.raises(ValueError, match="construct, point"):
        getattr(mod, opt_name)(_model(sym, shape, rank)[1], rank, 0.3, grad_at="bogus")


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("opt_name", OPTS)
def test_optimizers_descend_and_keep_the_manifold_at_the_point(sym, opt_name):
    """The loop and the criteria of test_riemannian.test_optimizers_descend_and_keep_the_manifold, grad_at="point"."""
    shape, rank = (6, 9, 9), (2, 3, 3)
    target = point(sym, seed=11, shape=shape, rank=rank).full()
    model, params, extract, mod = _model(sym, shape, rank)
    kw = {"RGD": {}, "RSGDwithMomentum": {"momentum_beta": 0.5}, "RiemannianAdam": {}}[opt_name]
    lr = 0.3 if opt_name != "RiemannianAdam" else 0.2
    opt = getattr(mod, opt_name)(params, rank, lr, grad_at="point", **kw)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.995)
    loss_fn = lambda T: 0.5 * ((T.full() - target) ** 2).sum()               # noqa: E731
    first = None
    for it in range(300):
        x_k = extract()
        gn = opt.fit(loss_fn, x_k, normalize_grad=False if opt_name != "RiemannianAdam" else 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        sched.step()
        first = opt.loss.item() if first is None else first
        assert torch.isfinite(gn)
    final = loss_fn(extract()).item()
    assert final < 0.05 * first, (first, final)
    for w in ([model.E.weight, model.R.weight] if sym else [model.S.weight, model.R.weight, model.O.weight]):
        assert (w.T @ w - torch.eye(w.shape[1], dtype=DT)).abs().max().item() < 1e-10
    assert opt.param_groups[0]["lr"] < lr


# ---- configuration -------------------------------------------------------------------------------------------------
def _cfg(rank, **train):
    from configs.base_config import Config
    cfg = Config(None)
    cfg.model_cfg.manifold_rank = rank
    for k, v in train.items():
        setattr(cfg.train_cfg, k, v)
    return cfg


def test_config_defaults_and_define_optimizer():
    from configs.base_config import TrainConfig, wn18rr_readme_config
    assert TrainConfig().grad_at == "construct" and TrainConfig().matrix_free is False
    tc = wn18rr_readme_config().train_cfg
    assert tc.grad_at == "construct" and tc.matrix_free is False
    rank = (2, 3, 3)
    for sym, mode in ((False, "asymmetric"), (True, "symmetric")):
        for name in ("rsgd", "rgd", "adam"):
            model = _model(sym, (6, 9, 9), rank)[0]
            assert driver.define_optimizer(model, _cfg(rank), mode, name).grad_at == "construct"
            assert driver.define_optimizer(model, _cfg(rank, grad_at="point"), mode, name).grad_at == "point"
            with pytest.raises(ValueError, match="construct, point"):
                driver.define_optimizer(model, _cfg(rank, grad_at="bogus"), mode, name)
    model = _model(False, (6, 9, 9), rank)[0]
    with pytest.raises(ValueError, match="grad_at=point"):
        driver.define_optimizer(model, _cfg((6, 112, 112), matrix_free=True), "asymmetric", "rsgd")


def test_step_config_refusals():
    driver.check_step_config("construct", False, (10, 200, 200))
    driver.check_step_config("point", True, (10, 200, 200))
    driver.check_step_config("point", True, (6, 208, 208))
    driver.check_step_config("construct", True, (6, 104, 104))            # doubled: 208, the edge of the range
    driver.check_step_config("point", True, (6, 212, 212))                # the kernels' own refusal, word for word
    with pytest.raises(ValueError, match="grad_at=point") as e:
        driver.check_step_config("construct", True, (6, 112, 112))
    assert "224" in str(e.value) and "208" in str(e.value)
    with pytest.raises(ValueError, match="construct, point"):
        driver.check_step_config("bogus", False, (6, 24, 24))


def _main(*overrides):
    import train
    argv = ["--mode", "asymmetric", "--optim", "rsgd", "--data", os.path.join(ROOT, "no-such-data") + "/",
            "--config", "wn18rr_readme", "--rank", "6", "112", "112"]
    for o in overrides:
        argv += ["--set", o]
    return train.main(argv)


def test_train_py_refuses_before_reading_the_data():
    with pytest.raises(SystemExit) as e:
        _main("train_cfg.grad_at=bogus")
    assert "construct, point" in str(e.value) and "bogus" in str(e.value)
    with pytest.raises(SystemExit) as e:
        _main("train_cfg.matrix_free=true")
    assert "grad_at=point" in str(e.value)
    with pytest.raises(SystemExit) as e:
        _main("train_cfg.matrix_free=true", "train_cfg.grad_at=construct")
    assert "grad_at=point" in str(e.value)
    with pytest.raises(SystemExit) as e:
        _main("train_cfg.matrix_free=perhaps")
    assert "true or false" in str(e.value)
    # accepted switches get as far as the data set, which is not there
    with pytest.raises(Exception) as e:
        _main("train_cfg.matrix_free=true", "train_cfg.grad_at=point")
    assert not isinstance(e.value, SystemExit)


def test_set_parses_the_bool_field():
    import train
    from configs.base_config import TrainConfig
    tc = TrainConfig()
    for raw, want in (("true", True), ("True", True), ("1", True), ("false", False), ("FALSE", False), ("0", False)):
        got = train._coerce(tc, "matrix_free", raw, f"train_cfg.matrix_free={raw}")
        assert got is want
    assert train._coerce(tc, "grad_at", "point", "train_cfg.grad_at=point") == "point"
    assert train._coerce(tc, "learning_rate", "1e-2", "x") == 0.01         # the other types as before


def test_captured_step_is_keyed_on_both_switches_and_hands_matrix_free_on():
    rank = (2, 3, 3)
    model, params, _, mod = _model(False, (6, 9, 9), rank)
    flt = types.SimpleNamespace(device=torch.device("cpu"))
    opt = mod.RSGDwithMomentum(params, rank, 0.3)
    s0 = driver._captured_step(model, opt, flt, 4, 0.1)
    assert driver._captured_step(model, opt, flt, 4, 0.1) is s0
    assert s0._loss_fn is driver.batch_loss_fn                              # the defaults: today's step
    s1 = driver._captured_step(model, opt, flt, 4, 0.1, "bce", True)
    assert s1 is not s0 and s1._loss_fn.keywords == {"matrix_free": True}
    s2 = driver._captured_step(model, opt, flt, 4, 0.1, "ce", True)
    assert s2._loss_fn.keywords == {"loss": "ce", "matrix_free": True}
    opt.grad_at = "point"
    s3 = driver._captured_step(model, opt, flt, 4, 0.1, "ce", True)
    assert s3 is not s2
    # refused before the first batch: the matrix-free loss at a construct of object rank 224
    big, bparams, _, _ = _model(False, (6, 120, 120), (6, 112, 112))
    bopt = mod.RSGDwithMomentum(bparams, (6, 112, 112), 0.3)
    with pytest.raises(ValueError, match="grad_at=point"):
        driver._captured_step(big, bopt, flt, 4, 0.1, "bce", True)
    driver._captured_step(big, bopt, flt, 4, 0.1, "bce", False)
