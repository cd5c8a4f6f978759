"""The float64 model of the relation-prediction gradients (tests/relation_grad_model.py) against torch.autograd, its
bounds against two wrong models, and the new entry points through ctypes on a machine without a GPU: every refusal is
a status code with the documented message, reported before a device is touched (the pointers are fakes)."""
import numpy as np
import pytest
import torch

import relation_grad_model as gm
from r_tucker_amd import _lib

RTK_ERR_BAD_ARG, RTK_ERR_WORKSPACE, RTK_ERR_UNSUPPORTED = -1, -2, -3
P = 0x10000        # a fake, 256-byte-aligned device pointer: never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def case():
    return gm.grad_case()


def test_model_equals_autograd(case):
    k = {n: torch.tensor(case[n], dtype=torch.float64, requires_grad=True) for n in ("core", "R", "S", "O")}
    h, t = torch.tensor(case["h"]), torch.tensor(case["t"])
    z = torch.einsum("ijk,dj,dk,ri->dr", k["core"], k["S"][h], k["O"][t], k["R"])
    z.backward(torch.tensor(case["dZ"], dtype=torch.float64))
    g = gm.gradients(*[case[n] for n in ("core", "R", "S", "O", "h", "t", "dZ")])
    for name, key in (("core", "gG"), ("R", "gR"), ("S", "gS"), ("O", "gO")):
        want = k[name].grad.numpy()
        assert np.abs(g[key] - want).max() <= 1e-12 * (1 + np.abs(want).max()), name
    assert np.abs(g["u"] @ case["R"].astype(np.float64).T - z.detach().numpy()).max() < 1e-10
    # the pieces agree with each other and with the bounds' values
    val, tau = gm.grad_bounds(*[case[n] for n in ("core", "R", "S", "O", "h", "t", "dZ")])
    assert all(np.array_equal(val[n], g[key]) for n, key in (("core", "gG"), ("R", "gR"), ("S", "gS"), ("O", "gO")))
    assert all((tau[n] >= 0).all() and np.isfinite(tau[n]).all() for n in tau)
    du = g["du"].astype(np.float32)
    assert np.allclose(gm.pair_rows(case["core"], case["O"], case["t"], g["du"]), g["rS"], rtol=1e-12, atol=1e-12)
    assert np.allclose(gm.core_outer(g["du"], case["S"][case["h"]].astype(np.float64), case["O"][case["t"]]), g["gG"])
    out, _ = gm.scatter_rows(case["h"], g["rS"], case["S"].shape[0])
    assert np.allclose(out, g["gS"], rtol=1e-12, atol=1e-12) and du.shape == g["du"].shape
    # the symmetric model: one table, the two gradients added
    vs, ts = gm.grad_bounds(case["core"], case["R"], case["S"], case["S"], case["h"], case["t"], case["dZ"], symmetric=True)
    E = torch.tensor(case["S"], dtype=torch.float64, requires_grad=True)
    zs = torch.einsum("ijk,dj,dk,ri->dr", k["core"].detach(), E[h], E[t], k["R"].detach())
    zs.backward(torch.tensor(case["dZ"], dtype=torch.float64))
    assert np.abs(vs["E"] - E.grad.numpy()).max() <= 1e-12 * (1 + np.abs(vs["E"]).max())
    assert (ts["E"] >= 0).all()


def test_bounds_can_fail(case):
    """A model with h and t exchanged in rS, and one with a single query dropped from gG, exceed the bounds on the
    inputs the GPU tests use."""
    args = [case[n] for n in ("core", "R", "S", "O", "h", "t", "dZ")]
    g = gm.gradients(*args)
    val, tau = gm.grad_bounds(*args)
    rS_bad = gm.pair_rows(case["core"], case["O"], case["h"], g["du"])            # O[h_d] in the place of O[t_d]
    gS_bad, _ = gm.scatter_rows(case["h"], rS_bad, case["S"].shape[0])
    assert (np.abs(gS_bad - val["S"]) > tau["S"]).any()
    d = 3
    gG_bad = val["core"] - np.einsum("i,j,k->ijk", g["du"][d], case["S"][case["h"][d]].astype(np.float64),
                                     case["O"][case["t"][d]].astype(np.float64))
    assert (np.abs(gG_bad - val["core"]) > tau["core"]).any()
    # ... and the same two mistakes against the kernels' own bounds on the cases of their tests
    core, X, idx, w = gm.rows_case(3, 5, 4, 33)
    rows, tau_r = gm.rows_bounds(core, X, idx, w)
    assert np.allclose(rows, gm.pair_rows(core, X, idx, w), rtol=1e-12, atol=1e-300)
    assert (np.abs(gm.pair_rows(core, X, np.roll(idx, 1), w) - rows) > tau_r).any()
    x, y, z = w, gm.rows_case(5, 3, 4, 33, 1)[3], X[idx]
    assert (np.abs(gm.core_outer(x[1:], y[1:], z[1:]) - gm.core_outer(x, y, z)) > gm.core_outer_bound(x, y, z)).any()


# ---- rtk_pair_rows_f32 --------------------------------------------------------------------------------------------
def _rows(lib, **kw):
    a = dict(core=P, a=10, b=200, c=200, X=P, n_x=100, idx=P, w=P, ld_w=None, batch=4, rows=P, ld_rows=None, ws=P,
             ws_bytes=1 << 30)
    a.update(kw)
    a["ld_w"] = a["a"] if a["ld_w"] is None else a["ld_w"]
    a["ld_rows"] = a["b"] if a["ld_rows"] is None else a["ld_rows"]
    rc = lib.rtk_pair_rows_f32(a["core"], a["a"], a["b"], a["c"], a["X"], a["n_x"], a["idx"], a["w"], a["ld_w"], a["batch"],
                               a["rows"], a["ld_rows"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(core=None), "null operand"),
    (dict(X=None), "null operand"),
    (dict(idx=None), "null operand"),
    (dict(w=None), "null operand"),
    (dict(rows=None), "null operand"),
    (dict(batch=-1), "batch = -1 must be >= 0"),
    (dict(a=0), "sizes must be positive"),
    (dict(b=0), "sizes must be positive"),
    (dict(c=0), "sizes must be positive"),
    (dict(n_x=0), "sizes must be positive"),
    (dict(ld_w=9), "ld_w = 9 below a = 10"),
    (dict(ld_rows=199), "ld_rows = 199 below b = 200"),
])
def test_rows_bad_arguments(lib, kw, msg):
    rc, err = _rows(lib, **kw)
    assert rc == RTK_ERR_BAD_ARG, (rc, err)
    assert msg in err and "rtk_pair_rows_f32" in err


@pytest.mark.parametrize("kw,msg", [
    (dict(c=212), "c = 212 above 208"),
    (dict(c=210), "c = 210 above 208"),
    (dict(c=18), "fp32 needs c % 4 == 0 and a 16-byte-aligned core (c = 18)"),
    (dict(core=P + 4), "16-byte-aligned core"),
    (dict(a=1 << 12, b=1 << 20), "dimension too large"),
])
def test_rows_unsupported_shapes(lib, kw, msg):
    rc, err = _rows(lib, **kw)
    assert rc == RTK_ERR_UNSUPPORTED, (rc, err)
    assert msg in err and "rtk_pair_rows_f32" in err


def test_rows_workspace(lib):
    f = lib.rtk_pair_rows_workspace_bytes
    assert f(0, 10, 200, 200) == 0 and f(-3, 10, 200, 200) == 0
    assert f(4, 0, 200, 200) == 0 and f(4, 10, 0, 200) == 0 and f(4, 10, 200, 0) == 0
    assert f(4, 10, 200, 212) == 0 and f(4, 10, 200, 18) == 0 and f(4, 1 << 12, 1 << 20, 200) == 0
    sizes = [f(B, 10, 200, 200) for B in (1, 32, 33, 512, 513, 2048, 8192)]
    assert all(s > 256 and s % 256 == 0 for s in sizes)
    assert all(x <= y for x, y in zip(sizes, sizes[1:])) and sizes[0] == sizes[1] < sizes[2] < sizes[3] < sizes[-1]
    # nothing of size B x a*b: the partial sums are a 32nd of it (a padded to 224), the rest grows with B (a + c)
    B, a, b, c = 2048, 200, 200, 200
    assert B * b * 224 * 4 // 32 <= f(B, a, b, c) < B * a * b * 4 // 8
    small = f(4, 10, 200, 200)
    rc, err = _rows(lib, ws_bytes=small - 1)
    assert rc == RTK_ERR_WORKSPACE and f"workspace of {small - 1} bytes given, {small} needed" in err, (rc, err)
    rc, err = _rows(lib, ws=None)
    assert rc == RTK_ERR_WORKSPACE and "workspace of 0 bytes given" in err, (rc, err)
    rc, err = _rows(lib, ws=P + 128, ws_bytes=small)
    assert rc == RTK_ERR_WORKSPACE and "workspace must be 256-byte aligned" in err, (rc, err)
    # batch == 0: a no-op, the per-batch pointers and the workspace may be missing ...
    rc, err = _rows(lib, batch=0, idx=None, w=None, rows=None, ws=None, ws_bytes=0)
    assert rc == 0, err
    # ... but not a way around the shape checks
    rc, err = _rows(lib, batch=0, c=600)
    assert rc == RTK_ERR_UNSUPPORTED and "c = 600 above 208" in err, err


# ---- rtk_core_outer_f32 -------------------------------------------------------------------------------------------
def _outer(lib, **kw):
    a = dict(x=P, ld_x=None, a=10, y=P, ld_y=None, b=20, z=P, ld_z=None, c=24, batch=4, gG=P)
    a.update(kw)
    for ld, n in (("ld_x", "a"), ("ld_y", "b"), ("ld_z", "c")):
        a[ld] = a[n] if a[ld] is None else a[ld]
    rc = lib.rtk_core_outer_f32(a["x"], a["ld_x"], a["a"], a["y"], a["ld_y"], a["b"], a["z"], a["ld_z"], a["c"], a["batch"],
                                a["gG"], None)
    return rc, lib.rtk_last_error_string().decode()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(x=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(y=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(z=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(gG=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(a=0), RTK_ERR_BAD_ARG, "sizes must be positive"),
    (dict(b=0), RTK_ERR_BAD_ARG, "sizes must be positive"),
    (dict(c=-1), RTK_ERR_BAD_ARG, "sizes must be positive"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "sizes must be positive"),
    (dict(ld_x=9), RTK_ERR_BAD_ARG, "ld_x = 9"),
    (dict(ld_y=19), RTK_ERR_BAD_ARG, "ld_y = 19"),
    (dict(ld_z=23), RTK_ERR_BAD_ARG, "ld_z = 23"),
    (dict(a=1 << 11, b=1 << 10, c=1 << 10), RTK_ERR_UNSUPPORTED, "dimension too large"),
    (dict(batch=1 << 31), RTK_ERR_UNSUPPORTED, "dimension too large"),
])
def test_outer_refusals(lib, kw, code, msg):
    rc, err = _outer(lib, **kw)
    assert rc == code, (rc, err)
    assert msg in err and "rtk_core_outer_f32" in err


# ---- rtk_scatter_rows_f32 -----------------------------------------------------------------------------------------
def _scatter(lib, **kw):
    a = dict(idx=P, rows=P, ld_rows=None, batch=4, n=36, n_out=60, out=P, ws=P, ws_bytes=1 << 30)
    a.update(kw)
    a["ld_rows"] = a["n"] if a["ld_rows"] is None else a["ld_rows"]
    rc = lib.rtk_scatter_rows_f32(a["idx"], a["rows"], a["ld_rows"], a["batch"], a["n"], a["n_out"], a["out"], a["ws"],
                                  a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(idx=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(rows=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(out=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1 must be >= 0"),
    (dict(n=0), RTK_ERR_BAD_ARG, "sizes must be positive"),
    (dict(n_out=0), RTK_ERR_BAD_ARG, "sizes must be positive"),
    (dict(ld_rows=35), RTK_ERR_BAD_ARG, "ld_rows = 35 below n = 36"),
    (dict(n=1025), RTK_ERR_UNSUPPORTED, "n = 1025 above 1024"),
    (dict(n_out=1 << 31), RTK_ERR_UNSUPPORTED, "dimension too large"),
    (dict(ws=None), RTK_ERR_WORKSPACE, "workspace of 0 bytes given"),
    (dict(ws=P + 128), RTK_ERR_WORKSPACE, "workspace must be 256-byte aligned"),
])
def test_scatter_refusals(lib, kw, code, msg):
    rc, err = _scatter(lib, **kw)
    assert rc == code, (rc, err)
    assert msg in err and "rtk_scatter_rows_f32" in err


def test_scatter_workspace(lib):
    f = lib.rtk_scatter_rows_workspace_bytes
    assert f(0) == 0 and f(-1) == 0 and f(1 << 31) == 0
    sizes = [f(B) for B in (1, 70, 512, 2048, 1 << 20)]
    assert all(s >= 256 and s % 256 == 0 for s in sizes) and all(x <= y for x, y in zip(sizes, sizes[1:]))
    rc, err = _scatter(lib, ws_bytes=sizes[0] - 1)
    assert rc == RTK_ERR_WORKSPACE and f"workspace of {sizes[0] - 1} bytes given, {sizes[0]} needed" in err, (rc, err)


def test_symbols_bound(lib):
    for name in ("rtk_pair_rows_workspace_bytes", "rtk_pair_rows_f32", "rtk_core_outer_f32",
                 "rtk_scatter_rows_workspace_bytes", "rtk_scatter_rows_f32"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    assert lib.rtk_version() == 214


def test_python_entry_points_refuse_cpu_tensors():
    import r_tucker_amd as rt
    core, R, E = torch.zeros(2, 4, 4, requires_grad=True), torch.zeros(4, 2), torch.zeros(5, 4)
    i0 = torch.tensor([0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.relation_logits(core, R, E, E, i0, i0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.relation_ce_loss(core, R, E, E, i0, i0, i0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.pair_rows(core.detach(), E, i0, torch.zeros(1, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.core_outer(torch.zeros(1, 2), torch.zeros(1, 4), torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.scatter_rows(i0, torch.zeros(1, 4), 5)
    for cls in (rt.AsymmetricR_TuckER, rt.SymmetricR_TuckER):
        m = cls((5, 4), (2, 4, 4))
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.relation_logits(i0, i0)
