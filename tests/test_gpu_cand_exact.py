"""Candidate scoring and its dv through the C ABI (rtk_score_candidates_{f32,bf16}, flags = 0, and
rtk_score_candidates_bwd_{f32,bf16} with gO = NULL), bit for bit against the float32 emulations of
tests/golden/cand_cases.py: the forward's lane layout, fmaf chain and xor butterfly, and dv's quarters of ceil(K / 4)
consecutive k with the combine ((p0 + p1) + p2) + p3.  The operands make every product a float32 number, so the
kernels' fmaf chains are chains of float32 adds and the outputs have to equal the emulations exactly; another order
changes the bits (tests/test_cand_cases_host.py proves that on the host).

Every call: the output inside a filled buffer with guards in front of it and behind it; the padding of dz and of out a
sentinel; dv's v all NaN (dv never reads it); dz NaN or inf where the id is invalid.  No tolerances.
"""
import numpy as np
import pytest
import torch

import cand_cases as cc

pytestmark = pytest.mark.gpu

GUARD = 64
by_name = dict(ids=lambda c: c.name)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def dev(a):
    t = torch.from_numpy(np.array(a, order="C")).cuda()                     # a copy: the cases' operands are read-only
    assert t.data_ptr() % 16 == 0
    return t


def shifted(values, off, fill=0.0):
    """-> (tensor, pointer): `values` (float32) on the device, its first element `off` floats behind a 16-byte
    boundary."""
    front = 4 + off
    t = dev(np.concatenate([np.full(front, fill, np.float32), np.asarray(values, np.float32).reshape(-1)]))
    ptr = t.data_ptr() + 4 * front
    assert (ptr % 16 == 0) == (off % 4 == 0)
    return t, ptr


def table(case):
    """-> (tensor, pointer) of O in the case's type, o_off elements behind a 16-byte boundary."""
    O = cc.operands(case).O
    front = 16 + case.o_off
    flat = np.concatenate([np.zeros(front, np.float32), O.reshape(-1)])
    t = dev(flat)
    if case.bf16:
        t16 = t.to(torch.bfloat16)
        assert torch.equal(t16.float(), t), "O does not hold bf16 values"
        t = t16
        assert t.data_ptr() % 16 == 0
    ptr = t.data_ptr() + t.element_size() * front
    assert (ptr % 16 == 0) == (case.o_off * t.element_size() % 16 == 0)
    assert (case.c % case.w == 0 and ptr % 16 == 0) == case.vector
    return t, ptr


def lists(case):
    op = cc.operands(case)
    d_cand = dev(op.cand if op.cand.size else np.zeros(1, np.int64))
    return d_cand, 0 if case.shared else case.K + case.cand_pad


def framed(rows, ld, off, fill):
    """A (rows x ld) float32 output `off` floats behind a 16-byte boundary inside a buffer filled with `fill`.
    -> (buffer, pointer, first index)."""
    front = GUARD + off
    buf = torch.full((front + rows * ld + GUARD,), fill, dtype=torch.float32, device="cuda")
    ptr = buf.data_ptr() + 4 * front
    assert buf.data_ptr() % 16 == 0 and (ptr % 16 == 0) == (off % 4 == 0)
    return buf, ptr, front


def unframe(buf, before, front, rows, ld, what):
    h = buf.cpu().numpy()
    assert np.array_equal(bits(h[:front]), bits(before[:front])), f"written in front of {what}"
    assert np.array_equal(bits(h[front + rows * ld:]), bits(before[front + rows * ld:])), f"written past {what}"
    return h[front:front + rows * ld].reshape(rows, ld)


def run_forward(lib, case):
    """-> out (B, ld_out) as the entry left it, the error word."""
    op = cc.operands(case)
    B, K, c, N = case.B, case.K, case.c, case.n_ent
    ld_out = K + case.out_pad
    d_cand, ld_cand = lists(case)
    d_v, v_ptr = shifted(op.v, case.v_off)
    d_O, O_ptr = table(case)
    buf, out_ptr, front = framed(B, ld_out, 0, float(cc.SENTINEL))
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    before = buf.cpu().numpy()
    fn = lib.rtk_score_candidates_bf16 if case.bf16 else lib.rtk_score_candidates_f32
    rc = fn(v_ptr, B, c, O_ptr, N, d_cand.data_ptr(), ld_cand, K, out_ptr, ld_out, 0, ws.data_ptr(), 256,
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    word = int(ws.cpu().numpy().view(np.uint32)[0])
    return unframe(buf, before, front, B, ld_out, "out"), word


def run_dv(lib, case, with_gO=False):
    """-> dv (B, c) as the entry left it, and gO (n_ent, c) when asked for.  Without gO: no workspace, and v all NaN."""
    op = cc.operands(case)
    B, K, c, N = case.B, case.K, case.c, case.n_ent
    d_cand, ld_cand = lists(case)
    d_dz = dev(op.dz if op.dz.size else np.zeros(1, np.float32))
    d_v, v_ptr = shifted(op.v if with_gO else np.full((max(B, 1), c), np.nan, np.float32), case.v_off, fill=np.nan)
    d_O, O_ptr = table(case)
    buf, dv_ptr, front = framed(B, c, case.dv_off, float("nan"))
    gbuf, g_ptr, gfront = framed(N, c, 0, float("nan"))
    nws = int(lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N)) if with_gO else 0
    ws = torch.full((max(nws, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    before, gbefore = buf.cpu().numpy(), gbuf.cpu().numpy()
    fn = lib.rtk_score_candidates_bwd_bf16 if case.bf16 else lib.rtk_score_candidates_bwd_f32
    rc = fn(d_dz.data_ptr(), K + case.dz_pad, v_ptr, B, c, O_ptr, N, d_cand.data_ptr(), ld_cand, K, dv_ptr,
            g_ptr if with_gO else None, ws.data_ptr() if with_gO else None, nws, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    dv = unframe(buf, before, front, B, c, "dv")
    gO = unframe(gbuf, gbefore, gfront, N, c, "gO")
    if not with_gO:
        assert np.array_equal(bits(gO), bits(gbefore[gfront:gfront + N * c].reshape(N, c)))
    return dv, gO


def run_gO_alone(lib, case):
    op = cc.operands(case)
    B, K, c, N = case.B, case.K, case.c, case.n_ent
    d_cand, ld_cand = lists(case)
    d_dz = dev(op.dz)
    d_v, v_ptr = shifted(op.v, case.v_off, fill=np.nan)
    d_O, O_ptr = table(case)
    gbuf, g_ptr, gfront = framed(N, c, 0, float("nan"))
    nws = int(lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N))
    ws = torch.full((max(nws, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    gbefore = gbuf.cpu().numpy()
    fn = lib.rtk_score_candidates_bwd_bf16 if case.bf16 else lib.rtk_score_candidates_bwd_f32
    rc = fn(d_dz.data_ptr(), K + case.dz_pad, v_ptr, B, c, O_ptr, N, d_cand.data_ptr(), ld_cand, K, None, g_ptr,
            ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    return unframe(gbuf, gbefore, gfront, N, c, "gO")


def forward_difference(case, got, ref):
    wrong = (bits(got) != bits(ref)) & ~(np.isnan(got) & np.isnan(ref))
    bad = np.argwhere(wrong)
    if not len(bad):
        return ""
    d, k = (int(x) for x in bad[0])
    span, nspan = cc.span_of(case.B, case.K)
    return (f"[{case.name}] {len(bad)} of {ref.size} scores differ; first at (d, k) = ({d}, {k}), entry {k % span} of "
            f"span {k // span} of {nspan}, id {int(cc.ids_of(case)[0][d, k])}: got {got[d, k]!r}, expected {ref[d, k]!r}")


def dv_difference(case, got, ref):
    """The count, the first element, the lane that holds it, and the wave (quarter) whose removal from the expected
    sum comes closest to what the kernel gave -- exact when one wave dropped its whole quarter."""
    bad = np.argwhere(bits(got) != bits(ref))
    if not len(bad):
        return ""
    d, j = (int(x) for x in bad[0])
    op = cc.operands(case)
    ids, ok = cc.ids_of(case)
    part = []
    for k0, k1 in cc.quarters(case.K):
        ks = [k for k in range(k0, k1) if ok[d, k]]
        part.append(sum(float(op.dz[d, k]) * float(op.O[ids[d, k], j]) for k in ks))
    gap = float(ref[d, j]) - float(got[d, j])
    if not np.isfinite(gap):
        owner = "not finite: an invalid id's dz was added"
    elif abs(gap) <= 2.0 ** -18 * sum(abs(p) for p in part):
        owner = "a difference of rounding size: the terms are there, their order is another"
    else:
        wave = int(np.argmin([abs(gap - p) for p in part]))
        owner = f"the difference is nearest to the share of wave {wave} (k in {cc.quarters(case.K)[wave]})"
    return (f"[{case.name}] {len(bad)} of {ref.size} elements of dv differ; first at (d, j) = ({d}, {j}), chunk "
            f"{j // case.W}, lane {j % case.W // case.w}, q {j % case.w}: got {got[d, j]!r}, expected {ref[d, j]!r}; "
            f"{owner}; quarters {cc.quarters(case.K)}")


@pytest.mark.parametrize("case", cc.cases_of("fwd"), **by_name)
def test_forward_bits(lib, case):
    out, word = run_forward(lib, case)
    K, ref = case.K, cc.expected_fwd(case)
    assert np.all(bits(out[:, K:]) == bits(cc.SENTINEL)), "the padding of out was written"
    got = out[:, :K]
    if case.B and K == 0:
        assert got.size == 0
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN exactly where the id is invalid"
    message = forward_difference(case, got, ref)
    assert not message, message
    assert word == cc.expected_error_word(case)


@pytest.mark.parametrize("case", cc.cases_of("dv"), **by_name)
def test_dv_bits(lib, case):
    got, _ = run_dv(lib, case)
    ref = cc.expected_dv(case)
    assert got.shape == ref.shape
    message = dv_difference(case, got, ref)
    assert not message, message


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_dv_and_gO_in_one_call(lib, bf16):
    """Both outputs together: dv keeps the emulation's bits, gO those of a call with dv = NULL."""
    case = cc.BY_NAME[cc.BOTH_OUTPUTS[bf16]]
    dv, gO = run_dv(lib, case, with_gO=True)
    message = dv_difference(case, dv, cc.expected_dv(case))
    assert not message, message
    alone = run_gO_alone(lib, case)
    assert np.isfinite(alone).all() and alone.any()
    bad = np.argwhere(bits(gO) != bits(alone))
    assert not len(bad), f"[{case.name}] {len(bad)} of {alone.size} elements of gO differ; first at {tuple(bad[0])}"
