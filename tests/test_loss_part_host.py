"""The block form of the matrix-free training loss without a GPU: the three ``rtk_bce_stream_*part*`` symbols, the
workspace-size function against the formula of its header comment, the argument checks of
``rtk_bce_stream_rows_part_f32`` / ``rtk_bce_stream_grad_o_part_f32`` (code and message before anything is enqueued)
and the Python entry point's refusal of CPU tensors."""
from types import SimpleNamespace

import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
SIG = _lib.RTK_SCORE_SIGMOID
NAMES = ("rtk_bce_stream_part_workspace_bytes", "rtk_bce_stream_rows_part_f32", "rtk_bce_stream_grad_o_part_f32")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, which, **kw):
    a = dict(qp=P, v=P, batch=4, c=16, O=P, n_local=40, col0=30, n_ent=100, slot=P, ptr=P, pobj=P, max_pos=64, eps=0.1,
             flags=SIG, scale=P, out=P, dv=None, ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    if which == "rows":
        rc = lib.rtk_bce_stream_rows_part_f32(a["qp"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"], a["n_ent"],
                                              a["slot"], a["ptr"], a["pobj"], a["eps"], a["flags"], a["out"], a["dv"],
                                              a["ws"], a["ws_bytes"], None)
    else:
        rc = lib.rtk_bce_stream_grad_o_part_f32(a["qp"], a["v"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"],
                                                a["n_ent"], a["slot"], a["ptr"], a["pobj"], a["max_pos"], a["eps"],
                                                a["flags"], a["scale"], a["out"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(slot=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ptr=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(pobj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(out=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(col0=-1), RTK_ERR_BAD_ARG, "col0 = -1"),
    (dict(n_local=0), RTK_ERR_BAD_ARG, "n_local = 0"),
    (dict(n_local=-3), RTK_ERR_BAD_ARG, "n_local = -3"),
    (dict(col0=61), RTK_ERR_BAD_ARG, "not a non-empty part of [0, n_ent = 100)"),       # 61 + 40 > 100
    (dict(n_local=101, col0=0), RTK_ERR_BAD_ARG, "not a non-empty part"),
    (dict(c=212), RTK_ERR_UNSUPPORTED, "c = 212 above 208"),
    (dict(c=6), RTK_ERR_UNSUPPORTED, "c % 4 == 0"),
    (dict(O=P + 4), RTK_ERR_UNSUPPORTED, "16-byte-aligned"),
    (dict(eps=1.0), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(eps=-0.5), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(flags=0), RTK_ERR_UNSUPPORTED, "RTK_SCORE_SIGMOID"),
    (dict(flags=SIG | 0x40), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(flags=SIG | _lib.RTK_SCORE_OUT_BF16), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(ws=WS + 64), RTK_ERR_BAD_ARG, "256-byte aligned"),
]


@pytest.mark.parametrize("which", ["rows", "grad_o"])
@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_refused_before_anything_is_enqueued(lib, which, kw, code, msg):
    rc, err = _call(lib, which, **kw)
    assert rc == code and msg in err, (rc, err)
    assert ("rtk_bce_stream_rows_part_f32" if which == "rows" else "rtk_bce_stream_grad_o_part_f32") in err


def test_the_last_row_of_the_matrix_is_a_valid_block_end(lib):
    """col0 + n_local == n_ent passes the block check (the call is then refused by a later one: a short workspace)."""
    for which in ("rows", "grad_o"):
        rc, err = _call(lib, which, col0=60, ws_bytes=255)
        assert rc == RTK_ERR_BAD_ARG and "255 bytes given" in err


def test_workspace_one_byte_short(lib):
    need_rows = lib.rtk_bce_stream_part_workspace_bytes(4, 40, 16, 0)
    need_go = lib.rtk_bce_stream_part_workspace_bytes(4, 40, 16, 64)
    assert 0 < need_rows < need_go
    for which, need in (("rows", need_rows), ("grad_o", need_go)):
        rc, err = _call(lib, which, ws_bytes=need - 1)
        assert rc == RTK_ERR_BAD_ARG and "needed" in err, (rc, err)
    # rows needs no list buffers: the max_pos = 0 size is enough for it and not for grad_o with max_pos = 64
    rc, err = _call(lib, "grad_o", ws_bytes=need_rows)
    assert rc == RTK_ERR_BAD_ARG and "needed" in err


def test_grad_o_own_arguments(lib):
    for kw, msg in ((dict(v=None), "null operand"), (dict(scale=None), "null operand"), (dict(max_pos=-1), "max_pos = -1")):
        rc, err = _call(lib, "grad_o", **kw)
        assert rc == RTK_ERR_BAD_ARG and msg in err


def test_rows_with_an_empty_batch_returns_at_once(lib):
    assert _call(lib, "rows", batch=0)[0] == 0


def _align256(x):
    return (x + 255) // 256 * 256


def _formula(lib, batch, c, max_pos):
    """The workspace formula of include/rtucker_hip.h (the comment above rtk_bce_stream_part_workspace_bytes)."""
    cp = 32 * ((c + 31) // 32)
    S = max(1, 256 // ((batch + 127) // 128))
    return (512 + _align256(8 * S * batch) + _align256(32 * batch) + _align256(4 * S * batch * cp) + 2 * _align256(4 * batch * c)
            + _align256(128 * cp * ((batch + 31) // 32)) + _align256(4 * (batch + 1)) + 3 * _align256(4 * max_pos)
            + _align256(lib.rtk_score_candidates_bwd_workspace_bytes(max_pos, 1, 1)))


def test_workspace_bytes(lib):
    f = lib.rtk_bce_stream_part_workspace_bytes
    assert f(-1, 100, 16, 0) == 0 and f(4, 0, 16, 0) == 0 and f(4, 100, 0, 0) == 0 and f(4, 100, 224, 0) == 0
    assert f(4, 100, 16, -1) == 0
    for batch, c, max_pos in ((4096, 200, 1_000_000), (70, 64, 630)):
        assert f(batch, 125_000, c, max_pos) == _formula(lib, batch, c, max_pos)
        # nothing grows with batch x n_local: the block's row count does not enter at all
        assert f(batch, 1_000, c, max_pos) == f(batch, 1_000_000, c, max_pos)
        # one layout for the block and the whole matrix
        assert f(batch, 1_000, c, max_pos) == lib.rtk_bce_stream_workspace_bytes(batch, 1_000_000, c, max_pos)
    assert f(4096, 125_000, 200, 1_000_000) < 4096 * 125_000 * 4 // 10


def test_symbols_bound(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]


def test_python_refusals_without_a_gpu():
    z = torch.zeros
    flt = SimpleNamespace(slot_of_item=torch.tensor([0]), pair_ptr=torch.tensor([0, 1]), pair_obj=torch.tensor([0]),
                          max_list=1)
    args = (z(2, 8, 8), z(3, 2), z(5, 8), z(3, 8), 2, 5, torch.tensor([0]), torch.tensor([0]), flt, torch.tensor([0]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.bce_loss_block_1vN(*args, label_smoothing=0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.ShardedEntityScorer(5).bce_loss_1vN(z(2, 8, 8), z(3, 2), z(5, 8), z(5, 8), torch.tensor([0]), torch.tensor([0]),
                                               flt, torch.tensor([0]), label_smoothing=0.1)
    import inspect
    ps = inspect.signature(rt.bce_loss_block_1vN).parameters
    assert list(ps)[:10] == ["core", "R", "S", "O_loc", "col0", "n_ent", "subject_idx", "relation_idx", "flt", "item_ids"]
    assert ps["all_reduce"].default is None and ps["max_pos"].default is None and ps["label_smoothing"].default == 0.0
    # bce_loss_1vN keeps its signature
    assert list(inspect.signature(rt.bce_loss_1vN).parameters) == [
        "core", "R", "S", "O", "subject_idx", "relation_idx", "flt", "item_ids", "label_smoothing", "matrix_free",
        "sigmoid_mode", "max_pos"]
