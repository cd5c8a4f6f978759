"""The block form of the matrix-free cross-entropy loss without a GPU: the three ``rtk_ce_stream_*part*`` symbols, the
workspace-size function, the argument checks of ``rtk_ce_stream_rows_part_f32`` / ``rtk_ce_stream_grad_part_f32`` (code
and message before anything is enqueued), the Python entry point's own checks, ``ce_merge_lse``, and the host logic of
``ops._CeLossBlock`` on float64 CPU stand-ins of its steps: over several partitions of the entities the blocks' shares
with ``lse = ce_merge_lse(...)`` must sum to ``F.cross_entropy``'s loss and gradients in float64."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import _lib, ops

# Stand-in device addresses: every call below is refused before a pointer is used.
P, WS = 1 << 20, 1 << 24
RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
NAMES = ("rtk_ce_stream_part_workspace_bytes", "rtk_ce_stream_rows_part_f32", "rtk_ce_stream_grad_part_f32")
FN = dict(rows="rtk_ce_stream_rows_part_f32", grad="rtk_ce_stream_grad_part_f32")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, which, **kw):
    a = dict(qp=P, v=P, batch=4, c=16, O=P, n_local=40, col0=30, n_ent=100, slot=P, ptr=P, pobj=P, max_pos=64, eps=0.1,
             lse=P, scale=P, m=P, s=P, lin=P, dv=P, gO=P, ws=WS, ws_bytes=1 << 30)
    a.update(kw)
    if which == "rows":
        rc = lib.rtk_ce_stream_rows_part_f32(a["qp"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"], a["n_ent"],
                                             a["slot"], a["ptr"], a["pobj"], a["eps"], a["m"], a["s"], a["lin"], a["ws"],
                                             a["ws_bytes"], None)
    else:
        rc = lib.rtk_ce_stream_grad_part_f32(a["qp"], a["v"], a["batch"], a["c"], a["O"], a["n_local"], a["col0"],
                                             a["n_ent"], a["slot"], a["ptr"], a["pobj"], a["max_pos"], a["eps"], a["lse"],
                                             a["scale"], a["dv"], a["gO"], a["ws"], a["ws_bytes"], None)
    return rc, lib.rtk_last_error_string().decode()


REFUSALS = [
    (dict(qp=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(O=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(slot=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ptr=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(pobj=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(ws=None), RTK_ERR_BAD_ARG, "null operand"),
    (dict(batch=-1), RTK_ERR_BAD_ARG, "batch = -1"),
    (dict(n_ent=0), RTK_ERR_BAD_ARG, "n_ent = 0"),
    (dict(c=0), RTK_ERR_BAD_ARG, "c = 0"),
    (dict(col0=-1), RTK_ERR_BAD_ARG, "col0 = -1"),
    (dict(n_local=0), RTK_ERR_BAD_ARG, "n_local = 0"),
    (dict(n_local=-3), RTK_ERR_BAD_ARG, "n_local = -3"),
    (dict(col0=61), RTK_ERR_BAD_ARG, "not a non-empty part of [0, n_ent = 100)"),       # 61 + 40 > 100
    (dict(n_local=101, col0=0), RTK_ERR_BAD_ARG, "not a non-empty part"),
    (dict(c=224), RTK_ERR_UNSUPPORTED, "c = 224 above 208"),
    (dict(c=212), RTK_ERR_UNSUPPORTED, "c = 212 above 208"),
    (dict(c=30), RTK_ERR_UNSUPPORTED, "c % 4 == 0"),
    (dict(O=P + 4), RTK_ERR_UNSUPPORTED, "16-byte-aligned"),
    (dict(eps=1.0), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(eps=-0.1), RTK_ERR_BAD_ARG, "label smoothing"),
    (dict(ws_bytes=255), RTK_ERR_BAD_ARG, "255 bytes given"),
    (dict(ws=WS + 64), RTK_ERR_BAD_ARG, "256-byte aligned"),
]


@pytest.mark.parametrize("which", ["rows", "grad"])
@pytest.mark.parametrize("kw,code,msg", REFUSALS)
def test_refused_before_anything_is_enqueued(lib, which, kw, code, msg):
    rc, err = _call(lib, which, **kw)
    assert rc == code and msg in err, (rc, err)
    assert FN[which] in err


def test_rows_part_own_arguments(lib):
    for kw in (dict(m=None), dict(s=None), dict(lin=None)):
        rc, err = _call(lib, "rows", **kw)
        assert rc == RTK_ERR_BAD_ARG and "null operand" in err, (kw, rc, err)
    rc, err = _call(lib, "rows", ws_bytes=lib.rtk_ce_stream_part_workspace_bytes(4, 40, 16, 0) - 1)
    assert rc == RTK_ERR_BAD_ARG and "needed" in err
    assert _call(lib, "rows", batch=0)[0] == 0                  # an empty batch returns at once


def test_grad_part_own_arguments(lib):
    # lse always; v and scale belong to gO_local_out; both outputs NULL is an error
    for kw in (dict(lse=None), dict(v=None), dict(scale=None), dict(dv=None, gO=None)):
        rc, err = _call(lib, "grad", **kw)
        assert rc == RTK_ERR_BAD_ARG and "null operand" in err, (kw, rc, err)
    rc, err = _call(lib, "grad", max_pos=-1)
    assert rc == RTK_ERR_BAD_ARG and "max_pos = -1" in err
    rc, err = _call(lib, "grad", ws_bytes=lib.rtk_ce_stream_part_workspace_bytes(4, 40, 16, 64) - 1)
    assert rc == RTK_ERR_BAD_ARG and "needed" in err
    # the rows size (max_pos = 0) is not enough for the list buffers of max_pos = 64
    rc, err = _call(lib, "grad", ws_bytes=lib.rtk_ce_stream_part_workspace_bytes(4, 40, 16, 0))
    assert rc == RTK_ERR_BAD_ARG and "needed" in err
    # without gO_local_out neither v nor scale is looked at: the call gets as far as the workspace check
    rc, err = _call(lib, "grad", gO=None, v=None, scale=None, ws_bytes=255)
    assert rc == RTK_ERR_BAD_ARG and "255 bytes given" in err


def test_the_last_row_of_the_matrix_is_a_valid_block_end(lib):
    for which in ("rows", "grad"):
        rc, err = _call(lib, which, col0=60, ws_bytes=255)
        assert rc == RTK_ERR_BAD_ARG and "255 bytes given" in err


def test_workspace_bytes(lib):
    f, whole = lib.rtk_ce_stream_part_workspace_bytes, lib.rtk_ce_stream_workspace_bytes
    assert f(-1, 100, 16, 0) == 0 and f(4, 0, 16, 0) == 0 and f(4, 100, 0, 0) == 0 and f(4, 100, 224, 0) == 0
    assert f(4, 100, 16, -1) == 0
    # the shapes of test_ce_stream_host.py::test_workspace_bytes
    for batch, c, max_pos in ((4, 16, 64), (1, 4, 0), (33, 100, 300), (70, 208, 630), (512, 200, 0), (4096, 200, 1_000_000)):
        want = whole(batch, 1000, c, max_pos)
        assert want > 0
        for n_local in (1000, 1_000_000):                    # n_local does not enter
            assert f(batch, n_local, c, max_pos) == want, (batch, c, max_pos, n_local)
    assert f(4096, 125_000, 200, 1_000_000) < 4096 * 125_000 * 4 // 10


def test_symbols_bound(lib):
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.SIGNATURES[name][0]
    import ctypes as C
    i64, p = C.c_int64, C.c_void_p
    assert _lib.SIGNATURES["rtk_ce_stream_rows_part_f32"][1] == [p, i64, C.c_int, p, i64, i64, i64, p, p, p, C.c_float, p, p, p,
                                                                 p, C.c_size_t, p]
    assert _lib.SIGNATURES["rtk_ce_stream_grad_part_f32"][1] == [p, p, i64, C.c_int, p, i64, i64, i64, p, p, p, i64, C.c_float,
                                                                 p, p, p, p, p, C.c_size_t, p]
    assert lib.rtk_version() == 214


# ---------------------------------------------------------------------------------------------- Python checks
def _tiny():
    z = torch.zeros
    flt = SimpleNamespace(slot_of_item=torch.tensor([0]), pair_ptr=torch.tensor([0, 1]), pair_obj=torch.tensor([0]),
                          max_list=1)
    return (z(2, 8, 8), z(3, 2), z(5, 8), z(3, 8), 2, 5, torch.tensor([0]), torch.tensor([0]), flt, torch.tensor([0]))


def test_python_mode_checks_without_a_gpu():
    args = _tiny()                                # rows [2, 5) of 5: a proper block

    def f(t):
        return t
    with pytest.raises(ValueError, match="not the loss"):
        rt.ce_loss_block_1vN(*args)                                              # neither, and not the whole range
    with pytest.raises(ValueError, match="come together"):
        rt.ce_loss_block_1vN(*args, all_reduce=f)                                # one collective without the other
    with pytest.raises(ValueError, match="come together"):
        rt.ce_loss_block_1vN(*args, all_reduce_max=f)
    with pytest.raises(ValueError, match="exclude each other"):
        rt.ce_loss_block_1vN(*args, all_reduce=f, all_reduce_max=f, lse=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        rt.ce_loss_block_1vN(*args, lse=torch.zeros(1, dtype=torch.float32))     # a float32 lse
    with pytest.raises(ValueError, match="float64"):
        rt.ce_loss_block_1vN(*args, lse=torch.zeros(2, dtype=torch.float64))     # not (B,)
    with pytest.raises(ValueError, match="float64"):
        rt.ce_loss_block_1vN(*args, lse=[0.0])
    # a right mode gets as far as the device check
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.ce_loss_block_1vN(*args, lse=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.ce_partials_block_1vN(*args)
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        rt.ShardedEntityScorer(5).ce_loss_1vN(z(2, 8, 8), z(3, 2), z(5, 8), z(5, 8), torch.tensor([0]), torch.tensor([0]),
                                              args[8], torch.tensor([0]), label_smoothing=0.1)


def test_signatures():
    ps = inspect.signature(rt.ce_loss_block_1vN).parameters
    assert list(ps) == ["core", "R", "S", "O_loc", "col0", "n_ent", "subject_idx", "relation_idx", "flt", "item_ids",
                        "label_smoothing", "max_pos", "all_reduce", "all_reduce_max", "lse"]
    assert all(ps[k].default is None for k in ("max_pos", "all_reduce", "all_reduce_max", "lse"))
    assert ps["label_smoothing"].default == 0.0
    assert list(inspect.signature(rt.ce_partials_block_1vN).parameters) == [
        "core", "R", "S", "O_loc", "col0", "n_ent", "subject_idx", "relation_idx", "flt", "item_ids", "label_smoothing"]
    assert list(inspect.signature(rt.ShardedEntityScorer.ce_loss_1vN).parameters) == [
        "self", "core", "R", "S", "O_loc", "subject_idx", "relation_idx", "flt", "item_ids", "label_smoothing", "max_pos",
        "partials_fn", "grad_fn", "stage1_bwd_fn"]
    # ce_loss_1vN keeps its signature
    assert list(inspect.signature(rt.ce_loss_1vN).parameters) == [
        "core", "R", "S", "O", "subject_idx", "relation_idx", "flt", "item_ids", "label_smoothing", "matrix_free", "max_pos"]


def test_merge_lse():
    rng = np.random.default_rng(5)
    z = torch.from_numpy(rng.standard_normal((7, 50)) * 40.0)
    z[3] += 900.0                                 # exp overflows without the maxima
    cuts = [0, 1, 18, 18, 50]                     # a block of one column and a block without columns
    ms, ss = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            m = z[:, a:b].max(dim=1).values
            ms.append(m.float().double())         # the kernel's m is a float; s is taken at that m
            ss.append(torch.exp(z[:, a:b] - ms[-1][:, None]).sum(dim=1))
        else:
            ms.append(torch.full((7,), float("-inf")))
            ss.append(torch.zeros(7, dtype=torch.float64))
    got = rt.ce_merge_lse(ms, ss)
    ref = torch.logsumexp(z, dim=1)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert (got - ref).abs().max() <= 1e-13 * ref.abs().max()
    with pytest.raises(ValueError):
        rt.ce_merge_lse([], [])


# ---------------------------------------------------------------------------------------------- the stand-in
TOL = 1e-10
EPS = 0.1
N_ENT, B, C_RANK, N_SUB = 23, 9, 8, 6


def _problem():
    """float64 operands: v = core-free stage 1 stand-in v[d] = S[h[d]] * R[r[d]] (elementwise, c columns)."""
    g = torch.Generator().manual_seed(11)
    S = torch.randn(N_SUB, C_RANK, generator=g, dtype=torch.float64)
    R = torch.randn(4, C_RANK, generator=g, dtype=torch.float64)
    core = torch.randn(C_RANK, generator=g, dtype=torch.float64)
    O = torch.randn(N_ENT, C_RANK, generator=g, dtype=torch.float64) * 2.0
    h = torch.randint(0, N_SUB, (B,), generator=g)
    r = torch.randint(0, 4, (B,), generator=g)
    # lists with entries in two blocks of every partition below (0 and 22; 5 and 6); one empty list; one of one entry
    lists = [[0, 22], [5, 6, 7], [], [3], [0, 5, 6, 22], [11, 12], [22], [1, 2, 21], [6]]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), dtype=torch.int64)
    obj = torch.tensor([x for l in lists for x in l], dtype=torch.int64)
    flt = SimpleNamespace(slot_of_item=torch.arange(B), pair_ptr=ptr, pair_obj=obj, max_list=4)
    y = torch.full((B, N_ENT), EPS / N_ENT, dtype=torch.float64)
    for d, l in enumerate(lists):
        if l:
            y[d, l] += (1.0 - EPS) / len(l)
    return core, R, S, O, h, r, flt, y, lists


def _qv(core, R, S, h, r):
    return S[h] * R[r] * core


def _ref(core, R, S, O, h, r, y):
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
    z = _qv(leaves[0], leaves[1], leaves[2], h, r) @ leaves[3].T
    loss = torch.nn.functional.cross_entropy(z, y)
    (3.0 * loss).backward()
    return loss.detach(), [t.grad for t in leaves], torch.logsumexp(z.detach(), dim=1)


def _targets(B_, O_loc, col0, n_ent, slot, ptr, obj, eps):
    """(y of the block's columns, the rows' mass w) by the kernels' rule: n_d is the whole list's length."""
    n = O_loc.shape[0]
    y = torch.full((B_, n), eps / n_ent, dtype=torch.float64)
    w = torch.full((B_,), eps, dtype=torch.float64)
    for d, s in enumerate(slot.tolist()):
        if s >= 0 and ptr[s + 1] > ptr[s]:
            l = obj[ptr[s]:ptr[s + 1]].tolist()
            w[d] += 1.0 - eps
            for e in l:
                if 0 <= e - col0 < n:
                    y[d, e - col0] += (1.0 - eps) / len(l)
    return y, w


def _cpu_partials(qp, B_, O_loc, col0, n_ent, slot, ptr, obj, eps):
    z = qp @ O_loc.detach().T
    y, _ = _targets(B_, O_loc, col0, n_ent, slot, ptr, obj, eps)
    m = z.max(dim=1).values
    return m, torch.exp(z - m[:, None]).sum(dim=1), -(y * z).sum(dim=1)


def _cpu_grad(qp, v, B_, O_loc, col0, n_ent, slot, ptr, obj, max_pos, eps, lse, scale, want_dv, want_gO):
    O_ = O_loc.detach()
    z = qp @ O_.T
    y, w = _targets(B_, O_loc, col0, n_ent, slot, ptr, obj, eps)
    x = w[:, None] * torch.exp(z - lse[:, None]) - y
    return (x @ O_ if want_dv else None), (x.T @ (v * scale) if want_gO else None)


def _cpu_stage1_bwd(core, R, S, h, r, dv, needs):
    leaves = [t.detach().clone().requires_grad_(True) for t in (core, R, S)]
    with torch.enable_grad():
        _qv(*leaves, h, r).backward(dv)
    return tuple(t.grad if n else None for t, n in zip(leaves, needs))


STEPS = SimpleNamespace(operands=lambda c_, R_, S_, O_, h, r, col0, n, who: (c_, R_, S_, O_, h.view(-1), r.view(-1)),
                        queries=lambda c_, R_, S_, h, r: (lambda v: (v, v))(_qv(c_.detach(), R_.detach(), S_.detach(), h, r)),
                        partials=_cpu_partials, grad=_cpu_grad, stage1_backward=_cpu_stage1_bwd)

PARTITIONS = {
    "one_block": [0, 23],
    "three_ragged": [0, 6, 19, 23],               # lists 1 and 4 have entries on both sides of 6
    "a_block_of_one_row": [0, 22, 23],            # the last block is entity 22 alone
    "a_block_without_a_positive": [0, 8, 11, 23],  # no list has an entry in [8, 11)
}


@pytest.mark.parametrize("name", list(PARTITIONS))
def test_shares_sum_to_the_loss(name):
    cuts = PARTITIONS[name]
    core, R, S, O, h, r, flt, y, lists = _problem()
    if name == "a_block_without_a_positive":
        assert not any(8 <= e < 11 for l in lists for e in l)
    assert any(len({sum(e >= c for c in cuts[1:-1]) for e in l}) > 1 for l in lists) or len(cuts) == 2
    ref_loss, ref_grads, ref_lse = _ref(core, R, S, O, h, r, y)
    items = torch.arange(B)
    blocks = list(zip(cuts[:-1], cuts[1:]))
    # every block's forward state, merged
    ms, ss = [], []
    slot = flt.slot_of_item[items]
    for a, b in blocks:
        m, s, _ = _cpu_partials(_qv(core, R, S, h, r), B, O[a:b], a, N_ENT, slot, flt.pair_ptr, flt.pair_obj, EPS)
        ms.append(m)
        ss.append(s)
    lse = rt.ce_merge_lse(ms, ss)
    assert (lse - ref_lse).abs().max() <= TOL * ref_lse.abs().max()
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S)]
    Oleaf = O.clone().requires_grad_(True)
    total = 0.0
    for a, b in blocks:
        share = ops._ce_block_loss(STEPS, *leaves, Oleaf[a:b], a, N_ENT, h, r, flt, items, EPS, None, None, None, lse)
        assert share.dtype == torch.float64
        (3.0 * share).backward()
        total = total + share.detach()
    assert abs(total - ref_loss) <= TOL * abs(ref_loss)
    for got, want in zip([t.grad for t in leaves] + [Oleaf.grad], ref_grads):
        assert got.shape == want.shape and (got - want).abs().max() <= TOL * want.abs().max()


def test_whole_range_without_lse_and_with_collectives():
    """The whole range needs nothing; with (identity) collectives the loss is the same and the exchanges are the three
    the issue names: MAX of (B,), SUM of (2, B), and SUM of (B, c) in the backward."""
    core, R, S, O, h, r, flt, y, _ = _problem()
    ref_loss, ref_grads, _ = _ref(core, R, S, O, h, r, y)
    items = torch.arange(B)
    seen = []
    for coll in (False, True):
        leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
        kw = (lambda t: seen.append(("sum", tuple(t.shape), t.dtype)), lambda t: seen.append(("max", tuple(t.shape), t.dtype))) \
            if coll else (None, None)
        loss = ops._ce_block_loss(STEPS, *leaves, 0, N_ENT, h, r, flt, items, EPS, None, kw[0], kw[1], None)
        (3.0 * loss).backward()
        assert abs(loss.detach() - ref_loss) <= TOL * abs(ref_loss)
        for got, want in zip([t.grad for t in leaves], ref_grads):
            assert (got - want).abs().max() <= TOL * want.abs().max()
    assert seen == [("max", (B,), torch.float64), ("sum", (2, B), torch.float64), ("sum", (B, C_RANK), torch.float64)]


def test_no_grad_and_empty_batch():
    core, R, S, O, h, r, flt, y, _ = _problem()
    calls = []
    steps = SimpleNamespace(**{**vars(STEPS), "grad": lambda *a: calls.append(1)})
    with torch.no_grad():
        loss = ops._ce_block_loss(steps, core, R, S, O, 0, N_ENT, h, r, flt, torch.arange(B), EPS, None, None, None, None)
    assert not loss.requires_grad and not calls
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
    e = torch.zeros(0, dtype=torch.int64)
    loss = ops._ce_block_loss(STEPS, *leaves, 0, N_ENT, e, e, flt, e, EPS, None, None, None, None)
    loss.backward()
    assert loss.item() == 0.0 and all(t.grad is not None and not t.grad.any() for t in leaves)


def test_a_block_without_rows_contributes_nothing():
    core, R, S, O, h, r, flt, y, _ = _problem()
    _, _, ref_lse = _ref(core, R, S, O, h, r, y)
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S)]
    O0 = O[:0].clone().requires_grad_(True)
    share = ops._ce_block_loss(STEPS, *leaves, O0, N_ENT, N_ENT, h, r, flt, torch.arange(B), EPS, None, None, None, ref_lse)
    share.backward()
    assert share.item() == 0.0 and O0.grad.shape == (0, C_RANK) and all(not t.grad.any() for t in leaves)
