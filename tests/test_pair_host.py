"""rtk_pair_vectors_* through ctypes on a machine without a GPU: every refusal is a status code with the documented
message, reported before a device is touched (the pointers are fakes: a call that got past the checks would fault),
and the workspace query is valid without a device."""
import pytest

from r_tucker_amd import _lib

RTK_ERR_BAD_ARG, RTK_ERR_WORKSPACE, RTK_ERR_UNSUPPORTED = -1, -2, -3
P = 0x10000        # a fake, 256-byte-aligned device pointer: never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, bf16=False, **kw):
    a = dict(core=P, a=10, b=200, c=200, S=P, n_subj=100, O=P, n_obj=100, h=P, t=P, batch=4, u=P, ld_u=None, packed=None,
             ws=P, ws_bytes=1 << 30)
    a.update(kw)
    if a["ld_u"] is None:
        a["ld_u"] = a["a"]
    fn = lib.rtk_pair_vectors_bf16 if bf16 else lib.rtk_pair_vectors_f32
    rc = fn(a["core"], a["a"], a["b"], a["c"], a["S"], a["n_subj"], a["O"], a["n_obj"], a["h"], a["t"], a["batch"], a["u"],
            a["ld_u"], a["packed"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kw,msg", [
    (dict(core=None), "null operand"),
    (dict(S=None), "null operand"),
    (dict(O=None), "null operand"),
    (dict(h=None), "null operand"),
    (dict(t=None), "null operand"),
    (dict(u=None), "null operand"),
    (dict(batch=-1), "batch = -1 must be >= 0"),
    (dict(a=0), "sizes must be positive"),
    (dict(b=0), "sizes must be positive"),
    (dict(c=0), "sizes must be positive"),
    (dict(n_subj=0), "sizes must be positive"),
    (dict(n_obj=0), "sizes must be positive"),
    (dict(ld_u=9), "ld_u = 9 below a = 10"),
])
def test_bad_arguments(lib, bf16, kw, msg):
    rc, err = _call(lib, bf16, **kw)
    assert rc == RTK_ERR_BAD_ARG, (rc, err)
    assert msg in err and ("rtk_pair_vectors_bf16" if bf16 else "rtk_pair_vectors_f32") in err


@pytest.mark.parametrize("kw,msg", [
    (dict(c=212), "c = 212 above 208"),
    (dict(c=210), "c = 210 above 208"),
    (dict(c=18), "fp32 needs c % 4 == 0 and a 16-byte-aligned core (c = 18)"),
    (dict(core=P + 4), "16-byte-aligned core"),
    (dict(a=600, packed=P), "packed planes of u need a <= 512"),
    (dict(a=1 << 20, b=1 << 12), "dimension too large"),
])
def test_f32_unsupported_shapes(lib, kw, msg):
    rc, err = _call(lib, **kw)
    assert rc == RTK_ERR_UNSUPPORTED, (rc, err)
    assert msg in err


def test_bf16_shapes(lib):
    rc, err = _call(lib, True, c=528)
    assert rc == RTK_ERR_UNSUPPORTED and "c = 528 above 512" in err, (rc, err)
    for c in (512, 18, 210):           # the bf16 sweep's shapes pass the checks up to the (too small) workspace
        rc, err = _call(lib, True, c=c, ws_bytes=256)
        assert rc == RTK_ERR_WORKSPACE and "256 bytes given" in err, (c, err)


@pytest.mark.parametrize("dtype", [0, 1])
def test_workspace(lib, dtype):
    f = lib.rtk_pair_vectors_workspace_bytes
    assert f(dtype, 0, 10, 200, 200) == 0 and f(dtype, -3, 10, 200, 200) == 0
    assert f(dtype, 4, 0, 200, 200) == 0 and f(dtype, 4, 10, 0, 200) == 0 and f(dtype, 4, 10, 200, 0) == 0
    assert f(2, 4, 10, 200, 200) == 0
    assert f(0, 4, 10, 200, 212) == 0 and f(0, 4, 10, 200, 18) == 0 and f(1, 4, 10, 200, 528) == 0
    sizes = [f(dtype, B, 10, 200, 200) for B in (1, 32, 33, 512, 513, 2048, 8192)]
    assert all(s > 256 and s % 256 == 0 for s in sizes)
    assert all(x <= y for x, y in zip(sizes, sizes[1:])) and sizes[0] == sizes[1] < sizes[2] < sizes[3] < sizes[-1]
    # nothing of size B x a*b: the partial sums are a 32nd of it (b padded to 224), the rest grows with B (b + c)
    B, a, b, c = 2048, 200, 200, 200
    need = f(dtype, B, a, b, c)
    assert B * a * 224 * 4 // 32 <= need < B * a * b * 4 // 8
    small = f(dtype, 4, 10, 200, 200)
    bf16 = dtype == 1
    rc, err = _call(lib, bf16, ws_bytes=small - 1)
    assert rc == RTK_ERR_WORKSPACE and f"workspace of {small - 1} bytes given, {small} needed" in err, (rc, err)
    rc, err = _call(lib, bf16, ws=None)
    assert rc == RTK_ERR_WORKSPACE and "workspace of 0 bytes given" in err, (rc, err)
    rc, err = _call(lib, bf16, ws=P + 128, ws_bytes=small)
    assert rc == RTK_ERR_WORKSPACE and "workspace must be 256-byte aligned" in err, (rc, err)
    # batch == 0: a no-op, the per-batch pointers and the workspace may be missing
    rc, err = _call(lib, bf16, batch=0, h=None, t=None, u=None, ws=None, ws_bytes=0)
    assert rc == 0, err
    # ... but not a way around the shape checks
    rc, err = _call(lib, bf16, batch=0, c=600)
    assert rc == RTK_ERR_UNSUPPORTED, err


def test_symbols_bound(lib):
    for name in ("rtk_pair_vectors_workspace_bytes", "rtk_pair_vectors_f32", "rtk_pair_vectors_bf16"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    assert _lib.SIGNATURES["rtk_pair_vectors_f32"] == _lib.SIGNATURES["rtk_pair_vectors_bf16"]
    assert lib.rtk_version() == 214


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    import r_tucker_amd as rt
    core, R, E = torch.zeros(2, 3, 3), torch.zeros(4, 2), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.pair_vectors(core, E, E, torch.tensor([0]), torch.tensor([0]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.score_relations(core, R, E, E, torch.tensor([0]), torch.tensor([0]))
    for cls in (rt.AsymmetricR_TuckER, rt.SymmetricR_TuckER):
        m = cls((5, 4), (2, 3, 3))
        assert callable(m.predict_relations) and callable(m.rank_relations)
