"""rtk_query_vectors_bwd_stream_f32 / _bf16 (csrc/rtk_query_bwd_stream.hip) through the C ABI.

The cases are those of tests/golden/stage1_bwd_stream_cases.py (proved on the host by
tests/test_stage1_bwd_stream_cases_host.py).  Exact cases: integer-valued operands with abs-sums below 2^24, so the
MFMA chains, the fma chains, the butterfly over the columns, the tile adds and the ordered scatter cannot round, and
g_core, g_R and g_S must equal the float64 result exactly.  Real cases: inside ``exact_cases.bwd_bounds(splits=1)``
(g_core is one chain over the batch); the largest error / bound is printed.  On every case g_S has the values of
rtk_query_vectors_bwd_f32 (the header's promise: the same chains) and g_core the bits of rtk_core_outer_f32 on the
gathered rows.  The _bf16 entry gives the bits of the _f32 entry on the same (bf16-exact) values.

Every call: outputs pre-filled with a sentinel (rows of absent ids come back exactly 0), workspace pre-filled with 0xFF
bytes, a second run bit-identical.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import exact_cases as ec
import stage1_bwd_stream_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
RTK_ERR_WORKSPACE, RTK_ERR_UNSUPPORTED = -2, -3
BY_NAME = {c.name: c for c in sc.CASES + [ec.BWD_NULL_CASE]}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


@functools.lru_cache(maxsize=None)
def operands_and_ref(name):
    """(operands, float64 reference) of a case: computed once, shared by the tests, never written to."""
    ops = ec.bwd_operands(BY_NAME[name])
    return ops, ec.bwd_ref(*ops)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Call:
    """Device copies of one case's operands and a fresh set of sentinel-filled outputs per run.  ``entry``: "stream_f32",
    "stream_bf16" (core, R, S stored as bf16) or "gemm" (rtk_query_vectors_bwd_f32)."""

    def __init__(self, lib, case, ops, entry="stream_f32"):
        self.lib, self.case, self.entry = lib, case, entry
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ops]
        if entry == "stream_bf16":
            for i in range(3):
                narrow = dev[i].to(torch.bfloat16)
                assert torch.equal(narrow.float(), dev[i]), "operand is not bf16-exact"
                dev[i] = narrow
        self.dev = dev
        size = lib.rtk_query_bwd_workspace_bytes if entry == "gemm" else lib.rtk_query_bwd_stream_workspace_bytes
        self.fn = {"gemm": lib.rtk_query_vectors_bwd_f32, "stream_f32": lib.rtk_query_vectors_bwd_stream_f32,
                   "stream_bf16": lib.rtk_query_vectors_bwd_stream_bf16}[entry]
        self.need = size(case.B, case.a, case.b, case.c)
        if entry != "gemm" and case.a <= 1024 and case.b <= 1024:
            assert 0 < self.need <= 64 * case.B * (case.a + case.b) + (1 << 20)

    def outputs(self):
        c = self.case
        return [torch.full(s, SENTINEL, dtype=torch.float32, device="cuda")
                for s in ((c.a, c.b, c.c), (c.n_rel, c.a), (c.n_sub, c.b))]

    def run(self, outs, want=(True, True, True), ws=None, ws_ptr=None, ws_bytes=None):
        c = self.case
        core, R, S, dv, rel, sub = self.dev
        if ws is None:
            ws = torch.full((max(self.need, 256),), 0xFF, dtype=torch.uint8, device="cuda")
            assert ws.data_ptr() % 256 == 0
        self.ws = ws
        ptrs = [o.data_ptr() if w else None for o, w in zip(outs, want)]
        rc = self.fn(core.data_ptr(), c.a, c.b, c.c, R.data_ptr(), c.n_rel, S.data_ptr(), c.n_sub, rel.data_ptr(),
                     sub.data_ptr(), c.B, dv.data_ptr(), *ptrs, ws.data_ptr() if ws_ptr is None else ws_ptr,
                     self.need if ws_bytes is None else ws_bytes, _stream())
        torch.cuda.synchronize()
        return rc


def first_difference(name, got, ref):
    bad = np.argwhere(got.astype(np.float64) != ref)
    i = tuple(bad[0])
    return f"{name}: {len(bad)} of {ref.size} elements differ; first at {i}: got {got[i]!r}, expected {ref[i]!r}"


def run_twice(lib, case, ops, entry="stream_f32"):
    call = Call(lib, case, ops, entry)
    res = []
    for _ in range(2):
        outs = call.outputs()
        rc = call.run(outs)
        assert rc == 0, lib.rtk_last_error_string()
        res.append([o.cpu().numpy() for o in outs])
    for x, y in zip(*res):
        assert np.array_equal(bits(x), bits(y)), "second run differs in its bits"
    return res[0]


def run_once(lib, case, ops, entry):
    call = Call(lib, case, ops, entry)
    outs = call.outputs()
    assert call.run(outs) == 0, lib.rtk_last_error_string()
    return [o.cpu().numpy() for o in outs]


def core_outer(lib, case, ops):
    """rtk_core_outer_f32 on the gathered rows R[r_d], S[h_d] and dv."""
    core, R, S, dv, rel, sub = ops
    x, y, z = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (R[rel], S[sub], dv)]
    out = torch.full((case.a, case.b, case.c), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.rtk_core_outer_f32(x.data_ptr(), case.a, case.a, y.data_ptr(), case.b, case.b, z.data_ptr(), case.c, case.c,
                                case.B, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.rtk_last_error_string()
    return out.cpu().numpy()


def check_against_neighbours(lib, case, ops, got):
    """g_S: the values of the GEMM form (a zero may differ in sign); g_core: the bits of rtk_core_outer_f32."""
    gemm = run_once(lib, case, ops, "gemm")
    assert np.array_equal(got[2], gemm[2]), f"[{case.branch}] g_S differs from rtk_query_vectors_bwd_f32's: " \
        + first_difference("g_S", got[2], gemm[2].astype(np.float64))
    assert np.array_equal(bits(got[0]), bits(core_outer(lib, case, ops))), "g_core differs from rtk_core_outer_f32's bits"


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.exact], ids=lambda c: c.name)
def test_stream_bwd_bit_exact(lib, case):
    ops, ref = operands_and_ref(case.name)
    got = run_twice(lib, case, ops)
    for name, g, e, ids in zip(("g_core", "g_R", "g_S"), got, ref, (None, ops[4], ops[5])):
        assert np.array_equal(g.astype(np.float64), e), f"[{case.branch}] " + first_difference(name, g, e)
        if ids is not None:                           # rows of ids absent from the batch: exactly zero, sentinel gone
            absent = np.setdiff1d(np.arange(g.shape[0]), ids)
            assert not g[absent].any()
    check_against_neighbours(lib, case, ops, got)


@pytest.mark.parametrize("case", [c for c in sc.CASES if not c.exact], ids=lambda c: c.name)
def test_stream_bwd_real_values_within_gamma_bounds(lib, case):
    ops, ref = operands_and_ref(case.name)
    bounds = ec.bwd_bounds(case, *ops, 1)
    got = run_twice(lib, case, ops)
    ratios = {}
    for name, g, e, bd in zip(("g_core", "g_R", "g_S"), got, ref, bounds):
        err = np.abs(g.astype(np.float64) - e)
        ratios[name] = float(np.max(err / np.maximum(bd, np.finfo(np.float64).tiny)))
    print(f"\n[stage-1 bwd stream real] {case.name}: max error / gamma bound: "
          + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for name, g, e, bd in zip(("g_core", "g_R", "g_S"), got, ref, bounds):
        assert np.isfinite(g).all() and np.all(np.abs(g.astype(np.float64) - e) <= bd), (name, ratios[name])
    check_against_neighbours(lib, case, ops, got)


@pytest.mark.parametrize("case", [c for c in sc.CASES if c.regime == "small" or not c.exact], ids=lambda c: c.name)
def test_bf16_entry_has_the_bits_of_the_f32_entry(lib, case):
    """core, R and S bf16-exact ("small": integers up to 2; real values rounded to 8 significant bits): the _bf16 entry
    on the bf16 storage and the _f32 entry on the same values as fp32 agree in every bit of every output."""
    ops, _ = operands_and_ref(case.name)
    if not case.exact:
        ops = tuple(ec.round_mantissa(x, 8) for x in ops[:3]) + ops[3:]
    wide = run_twice(lib, case, ops, "stream_f32")
    narrow = run_twice(lib, case, ops, "stream_bf16")
    for name, x, y in zip(("g_core", "g_R", "g_S"), wide, narrow):
        assert np.array_equal(bits(x), bits(y)), name
    if case.exact:
        for g, e in zip(narrow, ec.bwd_ref(*ops)):
            assert np.array_equal(g.astype(np.float64), e)


@pytest.mark.parametrize("entry", ["stream_f32", "stream_bf16"])
def test_null_outputs_every_subset(lib, entry):
    """Each output may be NULL: the others carry the bits of the full call, the skipped buffers keep their sentinel."""
    case = ec.BWD_NULL_CASE
    ops, ref = operands_and_ref(case.name)
    if entry == "stream_bf16":                        # the 12-bit dv stays fp32; core, R, S are signs: bf16-exact
        assert case.wide == "dv"
    call = Call(lib, case, ops, entry)
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
    ops, _ = operands_and_ref(case.name)
    call = Call(lib, case, ops)
    big = torch.full((call.need + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    for kw in (dict(ws_bytes=call.need - 1), dict(ws_bytes=0), dict(ws_ptr=0),
               dict(ws_ptr=big.data_ptr() + 128, ws_bytes=call.need), dict(ws_ptr=big.data_ptr() + 4, ws_bytes=call.need)):
        outs = call.outputs()
        assert call.run(outs, ws=big, **kw) == RTK_ERR_WORKSPACE, kw
        assert all(bool(torch.all(o == SENTINEL)) for o in outs), kw          # nothing written
        assert bool(torch.all(big == 0xFF)), kw                               # the workspace neither
    outs = call.outputs()
    assert call.run(outs, ws=big, ws_bytes=call.need) == 0                      # exactly the documented size is enough
    assert not any(bool(torch.any(o == SENTINEL)) for o in outs)
    assert bool(torch.all(big[call.need:] == 0xFF))                             # and nothing past it is written


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
