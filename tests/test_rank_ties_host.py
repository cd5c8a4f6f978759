"""The C entries of the tie-aware rank counts without a GPU: bindings, every refusal of the ranking entries' table
(tests/test_rank_host.py) for ``rtk_score_rank_tie_counts_*`` -- return code, message fragment and the function's name
in the message, before anything is enqueued -- the workspace query, and the argument checks of
``rtk_filtered_tie_counts_partial_f32`` and ``rtk_tie_metrics_f64``."""
import pytest

from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
SIG = _lib.RTK_SCORE_SIGMOID
TIE_ENTRIES = ("rtk_filtered_tie_counts_partial_f32", "rtk_score_rank_ties_workspace_bytes",
               "rtk_score_rank_tie_counts_f32", "rtk_score_rank_tie_counts_bf16", "rtk_tie_metrics_f64")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, bf16=False, **kw):
    a = dict(qp=P, batch=4, c=16, O=P, n_local=100, col0=0, n_ent=100, pt=P, obj=P, slot=None, ptr=None, pobj=None,
             flags=SIG, greater=P, equal=P, ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    fn = lib.rtk_score_rank_tie_counts_bf16 if bf16 else lib.rtk_score_rank_tie_counts_f32
    rc = fn(a["qp"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"], a["n_ent"], a["pt"], a["obj"], a["slot"],
            a["ptr"], a["pobj"], a["flags"], a["greater"], a["equal"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(obj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(pt=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(greater=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(equal=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(slot=P), RTK_ERR_BAD_ARG, "without the CSR arrays"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0, n_local=1), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(c=0), RTK_ERR_BAD_ARG, "c = 0"),
    (dict(col0=-1), RTK_ERR_BAD_ARG, "not a non-empty part"),
    (dict(n_local=0), RTK_ERR_BAD_ARG, "not a non-empty part"),
    (dict(col0=1), RTK_ERR_BAD_ARG, "not a non-empty part"),
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
    assert ("rtk_score_rank_tie_counts_bf16" if bf16 else "rtk_score_rank_tie_counts_f32") in err


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
    for c in (512, 18, 200):         # the bf16 kernel's shapes pass the checks up to the (too small) workspace
        rc, err = _call(lib, True, c=c, ws_bytes=256)
        assert rc == RTK_ERR_BAD_ARG and "256 bytes given" in err, (c, err)


def test_workspace_bytes(lib):
    f = lib.rtk_score_rank_ties_workspace_bytes
    part = lib.rtk_score_rank_part_workspace_bytes
    # 0 outside the covered range
    assert f(0, -1, 100, 200) == 0 and f(0, 4, 0, 200) == 0 and f(0, 4, 100, 0) == 0
    assert f(0, 4, 100, 212) == 0 and f(0, 4, 100, 18) == 0 and f(1, 4, 100, 513) == 0 and f(2, 4, 100, 16) == 0
    assert f(0, 4, 100, 208) > 0 and f(1, 4, 100, 18) > 0 and f(1, 4, 100, 512) > 0
    small, big = f(0, 512, 40943, 200), f(0, 8192, 40943, 200)
    assert 256 < small < big and small % 256 == 0
    assert small == part(0, 512, 40943, 200) == f(1, 512, 40943, 200)          # the block layout, whatever the dtype
    # nothing grows with batch x n_local: past the resident workgroups' rows the entity count does not matter
    assert f(0, 8192, 1_000_000, 200) == f(0, 8192, 125_000, 200) == f(1, 8192, 65536, 512) < 64 << 20
    rc, err = _call(lib, batch=512, n_local=40943, n_ent=40943, c=200, ws_bytes=small - 1)
    assert rc == RTK_ERR_BAD_ARG and f"{small} needed" in err
    # batch == 0: accepted (nothing enqueued) once the workspace holds the header
    rc, err = _call(lib, batch=0, ws_bytes=f(0, 0, 100, 16))
    assert rc == 0, err


def test_symbols_bound(lib):
    for name in TIE_ENTRIES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    assert _lib.SIGNATURES["rtk_score_rank_tie_counts_f32"] == _lib.SIGNATURES["rtk_score_rank_counts_f32"]
    assert _lib.SIGNATURES["rtk_filtered_tie_counts_partial_f32"] == _lib.SIGNATURES["rtk_filtered_rank_partial_f32"]
    assert lib.rtk_version() == 214


def _stored(lib, **kw):
    a = dict(P=P, batch=4, n_local=100, ld=100, col0=0, pt=P, obj=P, slot=None, ptr=None, pobj=None, greater=P, equal=P)
    a.update(kw)
    rc = lib.rtk_filtered_tie_counts_partial_f32(a["P"], a["batch"], a["n_local"], a["ld"], a["col0"], a["pt"], a["obj"],
                                                 a["slot"], a["ptr"], a["pobj"], a["greater"], a["equal"], None)
    return rc, lib.rtk_last_error_string().decode()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(P=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(pt=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(obj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(greater=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(equal=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=0), RTK_ERR_BAD_ARG, "bad sizes"),
    (dict(n_local=0), RTK_ERR_BAD_ARG, "bad sizes"),
    (dict(ld=99), RTK_ERR_BAD_ARG, "bad sizes"),
    (dict(col0=-1), RTK_ERR_BAD_ARG, "bad sizes"),
    (dict(slot=P), RTK_ERR_BAD_ARG, "without the CSR arrays"),
    (dict(batch=1 << 31), RTK_ERR_UNSUPPORTED, "dimension too large"),
    (dict(n_local=1 << 31, ld=1 << 31), RTK_ERR_UNSUPPORTED, "dimension too large"),
])
def test_stored_form_refusals(lib, kw, code, msg):
    rc, err = _stored(lib, **kw)
    assert rc == code, (rc, err)
    assert msg in err and "rtk_filtered_tie_counts_partial_f32" in err


@pytest.mark.parametrize("args", [(None, P, 4, P), (P, None, 4, P), (P, P, 4, None), (P, P, 0, P), (P, P, -3, P),
                                  (P, P, 1 << 31, P)])
def test_tie_metrics_refusals(lib, args):
    rc = lib.rtk_tie_metrics_f64(*args, None)
    assert rc == RTK_ERR_BAD_ARG and "rtk_tie_metrics_f64" in lib.rtk_last_error_string().decode()
