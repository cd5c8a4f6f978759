"""The matrix-free training loss without a GPU: the workspace-size function, the argument checks of
``rtk_bce_stream_rows_f32`` / ``rtk_bce_stream_grad_o_f32`` (code and message before anything is enqueued), the
bindings and the Python entry point's refusals."""
from types import SimpleNamespace

import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
SIG = _lib.RTK_SCORE_SIGMOID
NAMES = ("rtk_bce_stream_workspace_bytes", "rtk_bce_stream_rows_f32", "rtk_bce_stream_grad_o_f32")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, which, **kw):
    a = dict(qp=P, v=P, batch=4, c=16, O=P, n_ent=100, slot=P, ptr=P, pobj=P, max_pos=64, eps=0.1, flags=SIG, scale=P,
             out=P, dv=None, ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    if which == "rows":
        rc = lib.rtk_bce_stream_rows_f32(a["qp"], a["batch"], a["c"], a["O"], a["n_ent"], a["slot"], a["ptr"], a["pobj"],
                                         a["eps"], a["flags"], a["out"], a["dv"], a["ws"], a["ws_bytes"], None)
    else:
        rc = lib.rtk_bce_stream_grad_o_f32(a["qp"], a["v"], a["batch"], a["c"], a["O"], a["n_ent"], a["slot"], a["ptr"],
                                           a["pobj"], a["max_pos"], a["eps"], a["flags"], a["scale"], a["out"], a["ws"],
                                           a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(slot=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(pobj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(out=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(c=0), RTK_ERR_BAD_ARG, "c = 0"),
    (dict(eps=1.0), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(flags=0), RTK_ERR_UNSUPPORTED, "RTK_SCORE_SIGMOID"),
    (dict(flags=SIG | _lib.RTK_SCORE_OUT_BF16), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(flags=SIG | _lib.RTK_SCORE_KERNEL_WS), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(c=212), RTK_ERR_UNSUPPORTED, "c = 212 above 208"),
    (dict(c=224), RTK_ERR_UNSUPPORTED, "c = 224 above 208"),
    (dict(c=18), RTK_ERR_UNSUPPORTED, "c % 4 == 0"),
    (dict(O=P + 4), RTK_ERR_UNSUPPORTED, "16-byte-aligned"),
    (dict(ws_bytes=255), RTK_ERR_BAD_ARG, "255 bytes given"),
    (dict(ws=WS + 64), RTK_ERR_BAD_ARG, "256-byte aligned"),
]


@pytest.mark.parametrize("which", ["rows", "grad_o"])
@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_refused_before_anything_is_enqueued(lib, which, kw, code, msg):
    rc, err = _call(lib, which, **kw)
    assert rc == code and msg in err, (rc, err)


def test_grad_o_own_arguments(lib):
    for kw, msg in ((dict(v=None), "null operand"), (dict(scale=None), "null operand"), (dict(max_pos=-1), "max_pos = -1")):
        rc, err = _call(lib, "grad_o", **kw)
        assert rc == RTK_ERR_BAD_ARG and msg in err
    rc, err = _call(lib, "grad_o", ws_bytes=lib.rtk_bce_stream_workspace_bytes(4, 100, 16, 64) - 1)
    assert rc == RTK_ERR_BAD_ARG and "needed" in err


def test_rows_with_an_empty_batch_returns_at_once(lib):
    assert _call(lib, "rows", batch=0)[0] == 0


def test_workspace_bytes(lib):
    f = lib.rtk_bce_stream_workspace_bytes
    assert f(-1, 100, 16, 0) == 0 and f(4, 0, 16, 0) == 0 and f(4, 100, 0, 0) == 0 and f(4, 100, 224, 0) == 0
    assert f(4, 100, 16, -1) == 0
    small = f(4, 100, 16, 64)
    assert small > 0 and small % 256 == 0
    # no term grows with batch x n_ent: the entity count does not enter at all
    assert f(4096, 1_000_000, 200, 1_000_000) == f(4096, 1000, 200, 1_000_000)
    big = f(4096, 1_000_000, 200, 1_000_000)
    assert big < 4096 * 1_000_000 * 4 // 100                 # below 1 % of the matrix (164 MB)
    assert f(4096, 1_000_000, 200, 0) < big                  # the rows call alone needs no list buffers
    # splits is a function of the batch alone: 256 / ceil(batch / 128) slabs of batch x 224 floats
    assert f(512, 40943, 200, 0) >= 64 * 512 * 224 * 4
    assert f(512, 40943, 200, 0) < 64 * 512 * 224 * 4 + (4 << 20)


def test_symbols_bound(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_refusals_without_a_gpu():
    z = torch.zeros
    flt = SimpleNamespace(slot_of_item=torch.tensor([0]), pair_ptr=torch.tensor([0, 1]), pair_obj=torch.tensor([0]),
                          max_list=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.bce_loss_1vN(z(2, 8, 8), z(3, 2), z(5, 8), z(5, 8), torch.tensor([0]), torch.tensor([0]), flt,
                        torch.tensor([0]), label_smoothing=0.1, matrix_free=True)
    with pytest.raises(RuntimeError, match="no CPU path"):       # the autograd function itself: the whole matrix as one block
        rt.ops._BceLossBlock.apply(z(2, 8, 8), z(3, 2), z(5, 8), z(5, 8), torch.tensor([0]), torch.tensor([0]),
                                   torch.tensor([0]), torch.tensor([0, 1]), torch.tensor([0]), 0.1, None, 4, False, 0, 5,
                                   None, rt.ops._HipBlockLoss)
    assert "matrix_free" in rt.bce_loss_1vN.__code__.co_varnames
    import inspect
    from r_tucker_amd import driver
    assert inspect.signature(rt.bce_loss_1vN).parameters["matrix_free"].default is False
    assert inspect.signature(driver.batch_loss_fn).parameters["matrix_free"].default is False
