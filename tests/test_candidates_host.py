"""Candidate scoring without a GPU: the argument checks of the ``rtk_score_candidates*`` entries (return code and
message before anything is enqueued), their bindings, and the model methods refusing CPU tensors."""
import ctypes as C

import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _fwd(lib, bf16=False, **kw):
    a = dict(v=P, batch=4, c=16, O=P, n_ent=100, cand=P, ld_cand=8, k=8, out=P, ld_out=8, flags=0, ws=WS, ws_bytes=256)
    a.update(kw)
    fn = lib.rtk_score_candidates_bf16 if bf16 else lib.rtk_score_candidates_f32
    rc = fn(a["v"], a["batch"], a["c"], a["O"], a["n_ent"], a["cand"], a["ld_cand"], a["k"], a["out"], a["ld_out"],
            a["flags"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


def _bwd(lib, bf16=False, **kw):
    a = dict(dz=P, ld_dz=8, v=P, batch=4, c=16, O=P, n_ent=100, cand=P, ld_cand=8, k=8, dv=P, gO=P, ws=WS,
             ws_bytes=1 << 30)
    a.update(kw)
    fn = lib.rtk_score_candidates_bwd_bf16 if bf16 else lib.rtk_score_candidates_bwd_f32
    rc = fn(a["dz"], a["ld_dz"], a["v"], a["batch"], a["c"], a["O"], a["n_ent"], a["cand"], a["ld_cand"], a["k"], a["dv"],
            a["gO"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


FWD_REFUSALS = [
    (dict(v=None), "null operand"),
    (dict(O=None), "null operand"),
    (dict(cand=None), "null operand"),
    (dict(out=None), "null output"),
    (dict(c=0), "c = 0"),
    (dict(c=-3), "c = -3"),
    (dict(k=-1, ld_out=8), "must be >= 0"),
    (dict(batch=-1), "must be >= 0"),
    (dict(n_ent=0), "n_ent = 0"),
    (dict(ld_cand=5), "ld_cand = 5"),
    (dict(ld_out=7), "ld_out = 7"),
    (dict(flags=_lib.RTK_SCORE_OUT_BF16), "unknown flags"),
    (dict(flags=_lib.RTK_SCORE_EXACT_F32), "unknown flags"),
    (dict(flags=0x100), "unknown flags"),
    (dict(ws=None), "workspace"),
    (dict(ws_bytes=255), "255 bytes given"),
    (dict(ws=WS + 64), "256-byte aligned"),
]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kw,msg", FWD_REFUSALS)
def test_forward_refusals(lib, bf16, kw, msg):
    rc, err = _fwd(lib, bf16, **kw)
    assert rc == RTK_ERR_BAD_ARG, (rc, err)
    assert msg in err
    assert ("bf16" if bf16 else "f32") in err


BWD_REFUSALS = [
    (dict(dz=None), "null dZ"),
    (dict(v=None), "null operand"),
    (dict(O=None), "null operand"),
    (dict(cand=None), "null operand"),
    (dict(c=0), "c = 0"),
    (dict(k=-2), "must be >= 0"),
    (dict(n_ent=0), "n_ent = 0"),
    (dict(ld_cand=3), "ld_cand = 3"),
    (dict(ld_dz=7), "ld_dz = 7"),
    (dict(ws_bytes=1024), "1024 bytes given"),
    (dict(ws=None), "bytes given"),
    (dict(ws=WS + 8), "256-byte aligned"),
]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kw,msg", BWD_REFUSALS)
def test_backward_refusals(lib, bf16, kw, msg):
    rc, err = _bwd(lib, bf16, **kw)
    assert rc == RTK_ERR_BAD_ARG, (rc, err)
    assert msg in err


def test_unsupported_shapes(lib):
    rc, err = _fwd(lib, c=1025)
    assert rc == _lib.RTK_ERR_UNSUPPORTED if hasattr(_lib, "RTK_ERR_UNSUPPORTED") else rc == -3
    assert "1025" in err
    rc, err = _fwd(lib, batch=1 << 20, k=1 << 12, ld_cand=1 << 12, ld_out=1 << 12)
    assert rc == -3 and "2^31" in err


def test_backward_workspace_bytes(lib):
    f = lib.rtk_score_candidates_bwd_workspace_bytes
    assert f(0, 8, 100) == 0 and f(4, 0, 100) == 0 and f(4, 8, 0) == 0
    small, big = f(4, 8, 100), f(8192, 256, 1_000_000)
    assert 0 < small < big
    assert small % 256 == 0
    assert big < 48 * 8192 * 256 + (1 << 20) * 64        # O(B K): no (B, N) or (N, c) sized scratch
    # the gO workspace check uses this size
    rc, err = _bwd(lib, ws_bytes=small - 1)
    assert rc == RTK_ERR_BAD_ARG and f"{small} needed" in err


def test_symbols_bound(lib):
    for name in ("rtk_score_candidates_f32", "rtk_score_candidates_bf16", "rtk_score_candidates_bwd_f32",
                 "rtk_score_candidates_bwd_bf16", "rtk_score_candidates_bwd_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.rtk_version() == 214


def test_error_bit_message():
    """Bit 1 of the workspace error word is the candidate-id flag of _check_now."""
    import r_tucker_amd.ops as ops
    import inspect
    assert "candidate id out of range" in inspect.getsource(ops._check_now)


def _model_inputs(sym):
    n_ent, n_rel, rank = 20, 3, (2, 4, 4)
    if sym:
        model = rt.SymmetricR_TuckER((n_ent, n_rel), rank)
        model.init()
        T = rt.SFTucker(model.core.data, [model.R.weight.data], 2, model.E.weight.data)
    else:
        model = rt.AsymmetricR_TuckER((n_ent, n_rel), rank)
        model.init()
        T = rt.Tucker(model.core.data, [model.R.weight.data, model.S.weight.data, model.O.weight.data])
    return model, T


@pytest.mark.parametrize("sym", [False, True])
def test_model_methods_refuse_cpu_tensors(sym):
    model, T = _model_inputs(sym)
    h, r = torch.tensor([1, 2]), torch.tensor([0, 1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.score_candidates(h, r, torch.tensor([[1, 2, 3], [4, 5, 6]]))(T)
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.score_triples(h, r, torch.tensor([3, 4]))(T)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.score_candidates(T.core, T.factors[0], T.factors[1], T.factors[-1], h, r, torch.tensor([[1], [2]]))
