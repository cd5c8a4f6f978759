"""Matrix-free ranking on an entity block, without a GPU: the argument checks of ``rtk_score_rank_targets_*`` /
``rtk_score_rank_counts_*`` (return code and message before anything is enqueued), the workspace-size formula, the
bindings, and the Python entry points refusing CPU tensors and mismatched lengths."""
import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import _lib

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
SIG = _lib.RTK_SCORE_SIGMOID
NAMES = ("rtk_score_rank_part_workspace_bytes", "rtk_score_rank_targets_f32", "rtk_score_rank_targets_bf16",
         "rtk_score_rank_counts_f32", "rtk_score_rank_counts_bf16")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, step, bf16=False, **kw):
    a = dict(qp=P, batch=4, c=16, O=P, n_local=50, col0=25, n_ent=100, obj=P, pt=P, slot=None, ptr=None, pobj=None,
             flags=SIG, out=P, bce=None, ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    sfx = "_bf16" if bf16 else "_f32"
    if step == "targets":
        rc = getattr(lib, "rtk_score_rank_targets" + sfx)(a["qp"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"],
                                                          a["n_ent"], a["obj"], a["flags"], a["out"], a["ws"],
                                                          a["ws_bytes"], None)
    else:
        rc = getattr(lib, "rtk_score_rank_counts" + sfx)(a["qp"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"],
                                                         a["n_ent"], a["pt"], a["obj"], a["slot"], a["ptr"], a["pobj"],
                                                         a["flags"], a["out"], a["bce"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(obj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(out=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(col0=-1), RTK_ERR_BAD_ARG, "col0 = -1"),
    (dict(n_local=0), RTK_ERR_BAD_ARG, "n_local = 0"),
    (dict(n_local=-3), RTK_ERR_BAD_ARG, "n_local = -3"),
    (dict(col0=51), RTK_ERR_BAD_ARG, "col0 = 51, n_local = 50"),          # col0 + n_local = n_ent + 1
    (dict(n_local=101, col0=0), RTK_ERR_BAD_ARG, "n_local = 101"),
    (dict(c=0), RTK_ERR_BAD_ARG, "c = 0"),
    (dict(flags=0), RTK_ERR_UNSUPPORTED, "RTK_SCORE_SIGMOID"),
    (dict(flags=_lib.RTK_SCORE_SIGMOID_FAST), RTK_ERR_UNSUPPORTED, "RTK_SCORE_SIGMOID"),
    (dict(flags=SIG | _lib.RTK_SCORE_OUT_BF16), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(flags=SIG | _lib.RTK_SCORE_KERNEL_WS), RTK_ERR_BAD_ARG, "unknown flags"),
    (dict(ws_bytes=255), RTK_ERR_BAD_ARG, "255 bytes given"),
    (dict(ws=WS + 64), RTK_ERR_BAD_ARG, "256-byte aligned"),
]


@pytest.mark.parametrize("step", ["targets", "counts"])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_refusals(lib, step, bf16, kw, code, msg):
    rc, err = _call(lib, step, bf16, **kw)
    assert rc == code, (rc, err)
    assert msg in err
    assert ("rtk_score_rank_" + step + ("_bf16" if bf16 else "_f32")) in err


@pytest.mark.parametrize("bf16", [False, True])
def test_counts_only_refusals(lib, bf16):
    rc, err = _call(lib, "counts", bf16, pt=None)
    assert rc == RTK_ERR_BAD_ARG and "null operand" in err
    rc, err = _call(lib, "counts", bf16, slot=P)
    assert rc == RTK_ERR_BAD_ARG and "without the CSR arrays" in err
    rc, err = _call(lib, "counts", bf16, slot=P, ptr=P)
    assert rc == RTK_ERR_BAD_ARG and "without the CSR arrays" in err


@pytest.mark.parametrize("step", ["targets", "counts"])
@pytest.mark.parametrize("kw,msg", [
    (dict(c=210), "c = 210 above 208"),
    (dict(c=212), "c = 212 above 208"),
    (dict(c=18), "c % 4 == 0"),
    (dict(O=P + 4), "16-byte-aligned O"),
])
def test_f32_unsupported_shapes(lib, step, kw, msg):
    rc, err = _call(lib, step, **kw)
    assert rc == RTK_ERR_UNSUPPORTED, (rc, err)
    assert msg in err


@pytest.mark.parametrize("step", ["targets", "counts"])
def test_bf16_shapes(lib, step):
    rc, err = _call(lib, step, True, c=513)
    assert rc == RTK_ERR_UNSUPPORTED and "513" in err
    for c in (512, 18, 200):            # pass the checks up to the (too small) workspace
        rc, err = _call(lib, step, True, c=c, ws_bytes=256)
        assert rc == RTK_ERR_BAD_ARG and "256 bytes given" in err, (c, err)


def _formula(batch, n_local):
    """The header's formula: 256 + 2 align256(4 S batch) + 2 align256(4 * 8 * batch), S = min(512, ceil(n_local / 128))."""
    al = lambda x: (x + 255) // 256 * 256          # noqa: E731
    S = min(512, -(-n_local // 128))
    return 256 + 2 * al(4 * S * batch) + 2 * al(4 * 8 * batch)


def test_workspace_bytes(lib):
    f = lib.rtk_score_rank_part_workspace_bytes
    assert f(0, -1, 100, 200) == 0 and f(0, 4, 0, 200) == 0
    for dt, batch, n_local, c in [(0, 512, 40943, 200), (0, 500, 333, 36), (1, 2048, 14541, 200), (1, 8192, 125000, 512),
                                  (1, 8192, 1_000_000, 512), (0, 1, 1, 4), (0, 0, 100, 16)]:
        assert f(dt, batch, n_local, c) == _formula(batch, n_local), (dt, batch, n_local, c)
    shard = f(1, 8192, 125000, 512)
    assert shard < 64 << 20                              # the stored (B, n_local) fp32 block is 4.1 GB
    assert f(1, 8192, 1_000_000, 512) == f(1, 8192, 65536, 512)      # no term grows with batch * n_local
    small = f(0, 512, 40943, 200)
    rc, err = _call(lib, "counts", batch=512, n_local=40943, col0=0, n_ent=40943, c=200, ws_bytes=small - 1)
    assert rc == RTK_ERR_BAD_ARG and f"{small} needed" in err
    rc, err = _call(lib, "targets", batch=512, n_local=40943, col0=0, n_ent=40943, c=200, ws_bytes=small - 1)
    assert rc == RTK_ERR_BAD_ARG and f"{small} needed" in err
    # batch == 0: accepted (nothing enqueued) once the workspace holds the header
    for step in ("targets", "counts"):
        rc, err = _call(lib, step, batch=0, ws_bytes=f(0, 0, 50, 16))
        assert rc == 0, err


def test_symbols_bound(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert rt.rank_targets_block is rt.ops.rank_targets_block
    assert rt.rank_counts_block_1vN is rt.ops.rank_counts_block_1vN
    assert callable(rt.ShardedEntityScorer.rank_1vN)


def test_python_refuses_cpu_tensors_and_length_mismatches():
    qp = torch.zeros(4096, dtype=torch.uint8)
    O = torch.zeros(10, 16)
    t = torch.tensor([1, 2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.rank_targets_block(qp, 2, O, 0, 10, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.rank_counts_block_1vN(qp, 2, O, 0, 10, torch.zeros(2), t)
    with pytest.raises(TypeError):
        rt.rank_targets_block(qp, 2, None, 0, 10, t)


def test_block_operand_checks(monkeypatch):
    """The checks behind the two wrappers, run on CPU tensors with the device test switched off."""
    from r_tucker_amd import ops
    monkeypatch.setattr(ops, "_require_gpu", lambda name, t: None)
    O = torch.zeros(10, 16)
    qp = torch.zeros(ops._size("rtk_packed_query_bytes", 0, 2, 16), dtype=torch.uint8)
    b = ops._Block(qp, 2, O, 5, 20, torch.tensor([1, 2]))
    assert (b.B, b.n_loc, b.c, b.col0, b.n_ent, b.bf16) == (2, 10, 16, 5, 20, False)
    with pytest.raises(RuntimeError, match="object_idx has 3 entries for 2 queries"):
        ops._Block(qp, 2, O, 5, 20, torch.tensor([1, 2, 3]))
    with pytest.raises(RuntimeError, match="q_packed must be"):
        ops._Block(qp[:100], 2, O, 5, 20, torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="not a non-empty part"):
        ops._Block(qp, 2, O, 11, 20, torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="not a non-empty part"):
        ops._Block(qp, 2, O, -1, 20, torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops._Block(qp, 2, O.double(), 5, 20, torch.tensor([1, 2]))
    with pytest.raises(IndexError):
        ops._Block(qp, 2, O, 5, 20, torch.tensor([1.0, 2.0]))
    with pytest.raises(RuntimeError, match="pt must be"):
        ops.rank_counts_block_1vN(qp, 2, O, 5, 20, torch.zeros(3), torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="slots"):
        ops.rank_counts_block_1vN(qp, 2, O, 5, 20, torch.zeros(2), torch.tensor([1, 2]), flt=object())
    with pytest.raises(ValueError, match="slots need flt"):
        ops.rank_counts_block_1vN(qp, 2, O, 5, 20, torch.zeros(2), torch.tensor([1, 2]), slots=torch.tensor([0, 0]))
