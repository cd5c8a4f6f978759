"""The cross-entropy loss entries without a GPU: the workspace-size function and its closed form, the argument checks of
``rtk_ce_stream_rows_f32`` / ``rtk_ce_stream_grad_f32`` and of ``rtk_ce_rows_f32`` / ``rtk_ce_grad_f32`` (code and
message before anything is enqueued), and the bindings."""
import pytest

from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
NAMES = ("rtk_ce_stream_workspace_bytes", "rtk_ce_stream_rows_f32", "rtk_ce_stream_grad_f32", "rtk_ce_rows_f32",
         "rtk_ce_grad_f32")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, which, **kw):
    a = dict(qp=P, v=P, batch=4, c=16, O=P, n_ent=100, slot=P, ptr=P, pobj=P, max_pos=64, eps=0.1, lse=P, scale=P, out=P,
             dv=P, gO=P, ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    if which == "rows":
        rc = lib.rtk_ce_stream_rows_f32(a["qp"], a["batch"], a["c"], a["O"], a["n_ent"], a["slot"], a["ptr"], a["pobj"],
                                        a["eps"], a["out"], a["lse"], a["ws"], a["ws_bytes"], None)
    else:
        rc = lib.rtk_ce_stream_grad_f32(a["qp"], a["v"], a["batch"], a["c"], a["O"], a["n_ent"], a["slot"], a["ptr"],
                                        a["pobj"], a["max_pos"], a["eps"], a["lse"], a["scale"], a["dv"], a["gO"], a["ws"],
                                        a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(slot=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ptr=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(pobj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(lse=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(c=0), RTK_ERR_BAD_ARG, "c = 0"),
    (dict(eps=1.0), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(eps=-0.1), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(c=212), RTK_ERR_UNSUPPORTED, "c = 212 above 208"),
    (dict(c=224), RTK_ERR_UNSUPPORTED, "c = 224 above 208"),
    (dict(c=30), RTK_ERR_UNSUPPORTED, "c % 4 == 0"),
    (dict(O=P + 4), RTK_ERR_UNSUPPORTED, "16-byte-aligned"),
    (dict(ws_bytes=255), RTK_ERR_BAD_ARG, "255 bytes given"),
    (dict(ws=WS + 64), RTK_ERR_BAD_ARG, "256-byte aligned"),
]


@pytest.mark.parametrize("which", ["rows", "grad"])
@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_refused_before_anything_is_enqueued(lib, which, kw, code, msg):
    rc, err = _call(lib, which, **kw)
    assert rc == code and msg in err, (rc, err)


def test_rows_own_arguments(lib):
    rc, err = _call(lib, "rows", out=None)
    assert rc == RTK_ERR_BAD_ARG and "null operand" in err
    rc, err = _call(lib, "rows", ws_bytes=lib.rtk_ce_stream_workspace_bytes(4, 100, 16, 0) - 1)
    assert rc == RTK_ERR_BAD_ARG and "needed" in err
    assert _call(lib, "rows", batch=0)[0] == 0                  # an empty batch returns at once


def test_grad_own_arguments(lib):
    # v and scale belong to gO_out; both outputs NULL is an error, one of them is a sweep skipped
    for kw in (dict(v=None), dict(scale=None), dict(dv=None, gO=None)):
        rc, err = _call(lib, "grad", **kw)
        assert rc == RTK_ERR_BAD_ARG and "null operand" in err, (kw, rc, err)
    rc, err = _call(lib, "grad", max_pos=-1)
    assert rc == RTK_ERR_BAD_ARG and "max_pos = -1" in err
    rc, err = _call(lib, "grad", ws_bytes=lib.rtk_ce_stream_workspace_bytes(4, 100, 16, 64) - 1)
    assert rc == RTK_ERR_BAD_ARG and "needed" in err
    # without gO_out neither v nor scale is looked at: the call gets as far as the workspace check
    rc, err = _call(lib, "grad", gO=None, v=None, scale=None, ws_bytes=255)
    assert rc == RTK_ERR_BAD_ARG and "255 bytes given" in err


def _align256(x):
    return (x + 255) // 256 * 256


def _formula(lib, batch, c, max_pos):
    """The closed form of include/rtucker_hip.h."""
    cp = 32 * ((c + 31) // 32)
    n_mt = (batch + 31) // 32
    S = max(1, 256 // max(1, (n_mt + 3) // 4))
    a = _align256
    return (512 + a(4 * S * batch) + 2 * a(8 * S * batch) + a(32 * batch) + a(4 * S * batch * cp) + 2 * a(4 * batch * c)
            + a(128 * cp * n_mt) + a(256 * n_mt) + a(4 * (batch + 1)) + 3 * a(4 * max_pos)
            + a(lib.rtk_score_candidates_bwd_workspace_bytes(max_pos, 1, 1)))


def test_workspace_bytes(lib):
    f = lib.rtk_ce_stream_workspace_bytes
    assert f(-1, 100, 16, 0) == 0 and f(4, 0, 16, 0) == 0 and f(4, 100, 0, 0) == 0 and f(4, 100, 224, 0) == 0
    assert f(4, 100, 16, -1) == 0
    for batch, c, max_pos in ((4, 16, 64), (1, 4, 0), (33, 100, 300), (70, 208, 630), (512, 200, 0), (4096, 200, 1_000_000)):
        assert f(batch, 1000, c, max_pos) == _formula(lib, batch, c, max_pos), (batch, c, max_pos)
    # no term grows with batch x n_ent: the entity count does not enter at all
    assert f(4096, 1_000_000, 200, 1_000_000) == f(4096, 1000, 200, 1_000_000)
    big = f(4096, 1_000_000, 200, 1_000_000)
    assert big < 4096 * 1_000_000 * 4 // 100                 # below 1 % of the matrix (164 MB)
    assert f(4096, 1_000_000, 200, 0) < big                  # the forward needs no list buffers


def _matrix(lib, which, **kw):
    a = dict(Z=P, batch=4, n_ent=100, ld=128, slot=P, ptr=P, pobj=P, eps=0.1, rows=P, lse=P, g=P)
    a.update(kw)
    if which == "rows":
        rc = lib.rtk_ce_rows_f32(a["Z"], a["batch"], a["n_ent"], a["ld"], a["slot"], a["ptr"], a["pobj"], a["eps"],
                                 a["rows"], a["lse"], None)
    else:
        rc = lib.rtk_ce_grad_f32(a["Z"], a["batch"], a["n_ent"], a["ld"], a["slot"], a["ptr"], a["pobj"], a["eps"],
                                 a["lse"], a["g"], 0.25, None)
    return rc, lib.rtk_last_error_string().decode()


@pytest.mark.parametrize("which", ["rows", "grad"])
def test_matrix_form_refusals(lib, which):
    for kw, msg in ((dict(Z=None), "null operand"), (dict(slot=None), "null operand"), (dict(pobj=None), "null operand"),
                    (dict(batch=0), "bad sizes"), (dict(ld=99), "bad sizes"), (dict(eps=1.0), "label smoothing"),
                    (dict(lse=None), "null")):
        rc, err = _matrix(lib, which, **kw)
        assert rc == RTK_ERR_BAD_ARG and msg in err, (kw, rc, err)
    rc, err = _matrix(lib, which, **(dict(rows=None) if which == "rows" else dict(g=None)))
    assert rc == RTK_ERR_BAD_ARG and "null" in err
    if which == "grad":
        rc, err = _matrix(lib, which, batch=65536)
        assert rc == RTK_ERR_UNSUPPORTED and "65535" in err


def test_matrix_form_size_limits(lib):
    """One grid row per batch item in the gradient's launch; column indices are 32-bit."""
    rc, err = _matrix(lib, "grad", batch=65536)
    assert rc == RTK_ERR_UNSUPPORTED and "batch > 65535" in err
    assert _matrix(lib, "rows", batch=65536, n_ent=0)[0] == RTK_ERR_BAD_ARG       # (the rows entry has no such limit)
    for which in ("rows", "grad"):
        rc, err = _matrix(lib, which, n_ent=1 << 31, ld=1 << 31)
        assert rc == RTK_ERR_UNSUPPORTED and "dimension too large" in err, (which, rc, err)


def test_symbols_bound(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
