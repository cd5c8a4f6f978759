"""rtk_query_vectors_bwd_f32 (csrc/rtk_query_bwd.hip) through the C ABI, bit for bit against float64.

Operands come from tests/golden/exact_cases.py (integer-valued fp32, abs-sums below 2^24): the two GEMMs, the
per-query contractions of bwd_rows_kernel (fma chains and a shuffle tree) and the ordered adds of
scatter_rows_kernel cannot round, so g_core, g_R and g_S must equal the float64 result exactly -- a query dropped
from or counted twice in a list, a row added to the wrong id, an id compared on too few bits or an operand that
lost mantissa bits all show (proved on the host by tests/test_exact_cases_host.py).  One case per branch of the
kernels; `case.branch` names it.  A smaller real-valued layer is held to the derived bounds of
exact_cases.bwd_bounds; its largest error / bound is printed, never asserted against.

Every case: outputs pre-filled with a sentinel (rows of ids absent from the batch must come back exactly 0),
workspace pre-filled with 0xFF bytes, a second run bit-identical.  Out-of-range ids are not part of this file.
"""
import itertools

import numpy as np
import pytest
import torch

import exact_cases as ec

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
RTK_ERR_WORKSPACE, RTK_ERR_UNSUPPORTED = -2, -3


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Call:
    """Device copies of one case's operands and a fresh set of sentinel-filled outputs per run."""

    def __init__(self, lib, case, ops):
        self.lib, self.case = lib, case
        self.dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ops]
        self.need = lib.rtk_query_bwd_workspace_bytes(case.B, case.a, case.b, case.c)
        assert self.need >= 2 * case.B * case.a * case.b * 4

    def outputs(self):
        c = self.case
        return [torch.full(s, SENTINEL, dtype=torch.float32, device="cuda")
                for s in ((c.a, c.b, c.c), (c.n_rel, c.a), (c.n_sub, c.b))]

    def run(self, outs, want=(True, True, True), ws=None, ws_ptr=None, ws_bytes=None):
        c = self.case
        core, R, S, dv, rel, sub = self.dev
        if ws is None:
            ws = torch.full((self.need,), 0xFF, dtype=torch.uint8, device="cuda")
            assert ws.data_ptr() % 256 == 0
        ptrs = [o.data_ptr() if w else None for o, w in zip(outs, want)]
        rc = self.lib.rtk_query_vectors_bwd_f32(core.data_ptr(), c.a, c.b, c.c, R.data_ptr(), c.n_rel, S.data_ptr(), c.n_sub,
                                                rel.data_ptr(), sub.data_ptr(), c.B, dv.data_ptr(), *ptrs,
                                                ws.data_ptr() if ws_ptr is None else ws_ptr,
                                                ws.numel() if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc


def first_difference(name, got, ref):
    bad = np.argwhere(got.astype(np.float64) != ref)
    i = tuple(bad[0])
    return f"{name}: {len(bad)} of {ref.size} elements differ; first at {i}: got {got[i]!r}, expected {ref[i]!r}"


def run_twice(lib, case, ops):
    call = Call(lib, case, ops)
    res = []
    for _ in range(2):
        outs = call.outputs()
        rc = call.run(outs)
        assert rc == 0, lib.rtk_last_error_string()
        res.append([o.cpu().numpy() for o in outs])
    for x, y in zip(*res):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "second run differs in its bits"
    return res[0]


@pytest.mark.parametrize("case", [c for c in ec.BWD_CASES if c.exact], ids=lambda c: c.name)
def test_stage1_bwd_bit_exact(lib, case):
    ops = ec.bwd_operands(case)                       # asserts max abs-sum < 2^24 for g_core, g_R and g_S
    ref = ec.bwd_ref(*ops)
    got = run_twice(lib, case, ops)
    for name, g, e, ids in zip(("g_core", "g_R", "g_S"), got, ref, (None, ops[4], ops[5])):
        assert np.array_equal(g.astype(np.float64), e), f"[{case.branch}] " + first_difference(name, g, e)
        if ids is not None:                           # rows of ids absent from the batch: exactly zero, sentinel gone
            absent = np.setdiff1d(np.arange(g.shape[0]), ids)
            assert not g[absent].any()


@pytest.mark.parametrize("case", [c for c in ec.BWD_CASES if not c.exact], ids=lambda c: c.name)
def test_stage1_bwd_real_values_within_gamma_bounds(lib, case):
    ops = ec.bwd_operands(case)
    ref = ec.bwd_ref(*ops)
    splits = ec.gcore_splits(case.B, case.a, case.b, case.c)
    bounds = ec.bwd_bounds(case, *ops, splits)
    got = run_twice(lib, case, ops)
    ratios = {}
    for name, g, e, bd in zip(("g_core", "g_R", "g_S"), got, ref, bounds):
        err = np.abs(g.astype(np.float64) - e)
        ratios[name] = float(np.max(err / np.maximum(bd, np.finfo(np.float64).tiny)))
    print(f"\n[stage-1 bwd real] {case.name}: max error / gamma bound: "
          + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for name, g, e, bd in zip(("g_core", "g_R", "g_S"), got, ref, bounds):
        assert np.isfinite(g).all() and np.all(np.abs(g.astype(np.float64) - e) <= bd), (name, ratios[name])


def test_null_outputs_every_subset(lib):
    """Each output may be NULL: the others carry the bits of the full call, the skipped buffers keep their sentinel."""
    case = ec.BWD_NULL_CASE
    ops = ec.bwd_operands(case)
    ref = ec.bwd_ref(*ops)
    call = Call(lib, case, ops)
    full = call.outputs()
    assert call.run(full) == 0, lib.rtk_last_error_string()
    for g, e in zip(full, ref):
        assert np.array_equal(g.cpu().numpy().astype(np.float64), e)
    for want in itertools.product((False, True), repeat=3):
        outs = call.outputs()
        assert call.run(outs, want=want) == 0, (want, lib.rtk_last_error_string())
        for w, o, f in zip(want, outs, full):
            if w:
                assert torch.equal(o.view(torch.int32), f.view(torch.int32)), want
            else:
                assert torch.all(o == SENTINEL), want


def test_workspace_too_short_or_misaligned_is_refused(lib):
    case = ec.BWD_NULL_CASE
    call = Call(lib, case, ec.bwd_operands(case))
    big = torch.full((call.need + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    for kw in (dict(ws_bytes=call.need - 1), dict(ws_bytes=0), dict(ws_ptr=0),
               dict(ws_ptr=big.data_ptr() + 128, ws_bytes=call.need), dict(ws_ptr=big.data_ptr() + 4, ws_bytes=call.need)):
        outs = call.outputs()
        assert call.run(outs, ws=big, **kw) == RTK_ERR_WORKSPACE, kw
        assert all(bool(torch.all(o == SENTINEL)) for o in outs), kw          # nothing written
    outs = call.outputs()
    assert call.run(outs, ws=big, ws_bytes=call.need) == 0                      # exactly the documented size is enough
    assert not any(bool(torch.any(o == SENTINEL)) for o in outs)


@pytest.mark.parametrize("a,b", [(1025, 4), (4, 1025)])
def test_rank_1025_is_unsupported_and_outputs_untouched(lib, a, b):
    case = ec.BwdCase("rank_1025", 8, a, b, 4, 3, 5)
    ops = ec.bwd_operands(case)
    call = Call(lib, case, ops)
    outs = call.outputs()
    assert call.run(outs) == RTK_ERR_UNSUPPORTED
    assert all(bool(torch.all(o == SENTINEL)) for o in outs)
    ok = ec.BwdCase("rank_1024", 8, min(a, 1024), min(b, 1024), 4, 3, 5)      # one less is taken (and exact)
    ops = ec.bwd_operands(ok)
    got = run_twice(lib, ok, ops)
    for g, e in zip(got, ec.bwd_ref(*ops)):
        assert np.array_equal(g.astype(np.float64), e)
