"""Filtered ranking without the score matrix, without a GPU: the argument checks of ``rtk_score_rank_*`` (return code
and message before anything is enqueued), the workspace-size query, the bindings, and the Python entry points refusing
CPU tensors and mismatched object ids."""
import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
SIG = _lib.RTK_SCORE_SIGMOID


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, bf16=False, **kw):
    a = dict(qp=P, batch=4, c=16, O=P, n_ent=100, obj=P, slot=None, ptr=None, pobj=None, flags=SIG, ranks=P, bce=None,
             ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    fn = lib.rtk_score_rank_bf16 if bf16 else lib.rtk_score_rank_f32
    rc = fn(a["qp"], a["batch"], a["c"], a["O"], a["n_ent"], a["obj"], a["slot"], a["ptr"], a["pobj"], a["flags"],
            a["ranks"], a["bce"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(obj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ranks=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(slot=P), RTK_ERR_BAD_ARG, "without the CSR arrays"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(c=0), RTK_ERR_BAD_ARG, "c = 0"),
    (dict(flags=0), RTK_ERR_UNSUPPORTED, "RTK_SCORE_SIGMOID"),
    (dict(flags=_lib.RTK_SCORE_SIGMOID_FAST), RTK_ERR_UNSUPPORTED, "RTK_SCORE_SIGMOID"),
    (dict(flags=SIG | _lib.RTK_SCORE_OUT_BF16), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(flags=SIG | _lib.RTK_SCORE_KERNEL_WS), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(ws_bytes=255), RTK_ERR_BAD_ARG, "255 bytes given"),
    (dict(ws=WS + 64), RTK_ERR_BAD_ARG, "256-byte aligned"),
]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_refusals(lib, bf16, kw, code, msg):
    rc, err = _call(lib, bf16, **kw)
    assert rc == code, (rc, err)
    assert msg in err
    assert ("bf16" if bf16 else "f32") in err


@pytest.mark.parametrize("kw,msg", [
    (dict(c=210), "c = 210 above 208"),
    (dict(c=212), "c = 212 above 208"),
    (dict(c=18), "c % 4 == 0"),
    (dict(O=P + 4), "16-byte-aligned O"),
])
def test_f32_unsupported_shapes(lib, kw, msg):
    rc, err = _call(lib, **kw)
    assert rc == RTK_ERR_UNSUPPORTED, (rc, err)
    assert msg in err


def test_bf16_shapes(lib):
    rc, err = _call(lib, True, c=513)
    assert rc == RTK_ERR_UNSUPPORTED and "513" in err
    # c = 512 and c % 4 != 0 are the bf16 kernel's; they pass the checks up to the (too small) workspace
    for c in (512, 18, 200):
        rc, err = _call(lib, True, c=c, ws_bytes=256)
        assert rc == RTK_ERR_BAD_ARG and "256 bytes given" in err, (c, err)


def test_workspace_bytes(lib):
    f = lib.rtk_score_rank_workspace_bytes
    assert f(0, -1, 100, 200) == 0 and f(0, 4, 0, 200) == 0
    small, big = f(0, 512, 40943, 200), f(0, 8192, 40943, 200)
    assert 256 < small < big and small % 256 == 0
    assert f(1, 512, 40943, 200) == small
    assert f(1, 8192, 1_000_000, 512) < 64 << 20          # O(B) scratch: no (B, N) matrix
    rc, err = _call(lib, batch=512, n_ent=40943, c=200, ws_bytes=small - 1)
    assert rc == RTK_ERR_BAD_ARG and f"{small} needed" in err
    # batch == 0: accepted (nothing enqueued) once the workspace holds the header
    rc, err = _call(lib, batch=0, ws_bytes=f(0, 0, 100, 16))
    assert rc == 0, err


def test_symbols_bound(lib):
    for name in ("rtk_score_rank_f32", "rtk_score_rank_bf16", "rtk_score_rank_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_error_bit_message():
    """Bit 2 of the workspace error word is the object-id flag of _check_now."""
    import inspect
    import r_tucker_amd.ops as ops
    src = inspect.getsource(ops._check_now)
    assert "flag.value & 4" in src and "object_idx" in src


def _model(sym):
    n_ent, n_rel, rank = 20, 3, (2, 4, 4)
    model = (rt.SymmetricR_TuckER if sym else rt.AsymmetricR_TuckER)((n_ent, n_rel), rank)
    model.init()
    return model


@pytest.mark.parametrize("sym", [False, True])
def test_refuse_cpu_tensors(sym):
    model = _model(sym)
    h, r, t = torch.tensor([1, 2]), torch.tensor([0, 1]), torch.tensor([3, 4])
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.rank_objects(h, r, t)
    S = model.E.weight if sym else model.S.weight
    O = model.E.weight if sym else model.O.weight
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.rank_1vN(model.core, model.R.weight, S, O, h, r, t)


@pytest.mark.parametrize("sym", [False, True])
def test_object_idx_length_checked(sym):
    model = _model(sym)
    h, r = torch.tensor([1, 2]), torch.tensor([0, 1])
    with pytest.raises(RuntimeError, match="object_idx has 3 entries for 2 queries"):
        model.rank_objects(h, r, torch.tensor([3, 4, 5]))
    S = model.E.weight if sym else model.S.weight
    O = model.E.weight if sym else model.O.weight
    with pytest.raises(RuntimeError, match="object_idx has 1 entries for 2 queries"):
        rt.rank_1vN(model.core, model.R.weight, S, O, h, r, torch.tensor([3]))
