"""The matrix-form BCE loss kernels through their four C entry points, on inputs built here: rtk_bce_rows_f32 and
rtk_bce_grad_f32 on planted score rows, rtk_bce_patch_pos_f32 on exact logits, rtk_score_packed_bce_f32 against
rtk_score_packed_f32 on the same packed planes.  No stage 1 and no GEMM enters any bound.

Cases, references and bounds: tests/golden/bce_cases.py (proved on the host by tests/test_bce_cases_host.py).  Row sums
are held to the derived bound against float64, gradients and stored values to their bit patterns; the largest
error / bound of every case is printed.  Row padding (ld > N) is NaN before and must be the same NaN afterwards.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_cases as bc

pytestmark = pytest.mark.gpu

RTK_ERR_BAD_ARG, RTK_ERR_UNSUPPORTED = -1, -3
SIGMOID, SIGMOID_FAST, KERNEL_V3 = 1, 4, 0x300
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def csr_dev(csr):
    return dev(csr.slot), dev(csr.ptr), dev(csr.obj)


def setup_rows(case):
    csr = bc.build_csr(np.random.default_rng(bc._seed(case.name)), case.N, case.lengths, case.B)
    P, pos = bc.plant(case, csr)
    return csr, P, pos


# ---------------------------------------------------------------------------------------------- rows ------
@pytest.mark.parametrize("case", bc.ROWS_CASES, ids=lambda c: c.name)
def test_rows_against_float64(lib, case):
    csr, P, pos = setup_rows(case)
    ref, mag = bc.rows_reference(case, P, pos)
    bound = bc.rows_bound(case.N, max(case.lengths), mag, ref)
    own = (-(-case.N // 256) + -(-max(case.lengths) // 256) + 16) * bc.U * mag + case.N * 2.0 ** -23
    slot, ptr, obj = csr_dev(csr)
    Pd = dev(P)
    runs = []
    for _ in range(2):
        rows = torch.full((case.B + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib.rtk_bce_rows_f32(Pd.data_ptr(), case.B, case.N, case.ld, slot.data_ptr(), ptr.data_ptr(), obj.data_ptr(),
                                  case.eps, rows.data_ptr(), _stream())
        assert rc == 0, lib.rtk_last_error_string()
        torch.cuda.synchronize()
        runs.append(rows.cpu().numpy())
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64)), "second run differs in its bits"
    got = runs[0][:case.B]
    assert np.isnan(runs[0][case.B:]).all(), "written past row B"
    assert np.array_equal(bits(Pd.cpu().numpy()), bits(P)), "P was written"
    err = np.abs(got - ref)
    print(f"\n[bce rows] {case.name}: max error / derived bound = {float((err / own).max()):.4f}, "
          f"/ asserted bound = {float((err / bound).max()):.4f}")
    assert np.isfinite(got).all() and np.all(err <= bound), \
        f"row {int(np.argmax(err / bound))}: got {got[np.argmax(err / bound)]!r}, expected {ref[np.argmax(err / bound)]!r}"


# ---------------------------------------------------------------------------------------------- grad ------
@pytest.mark.parametrize("case", bc.GRAD_CASES, ids=lambda c: c.name)
def test_grad_bit_for_bit(lib, case):
    csr, P, pos = setup_rows(case)
    ref = bc.grad_reference(case, P, pos)
    slot, ptr, obj = csr_dev(csr)
    g = dev(np.array([bc.GRAD_G], dtype=np.float32))
    flat = np.concatenate([np.full(case.off, np.nan, np.float32), P.reshape(-1), np.full(GUARD, np.nan, np.float32)])
    buf = dev(flat)
    p_ptr = buf.data_ptr() + 4 * case.off
    assert ((case.ld % 4 == 0) and p_ptr % 16 == 0) == (case.ld % 4 == 0 and case.off % 4 == 0)
    rc = lib.rtk_bce_grad_f32(p_ptr, case.B, case.N, case.ld, slot.data_ptr(), ptr.data_ptr(), obj.data_ptr(), case.eps,
                              g.data_ptr(), 1.0 / (case.B * case.N), _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    body = h[case.off:case.off + case.B * case.ld].reshape(case.B, case.ld)
    assert np.array_equal(bits(h[:case.off]), bits(flat[:case.off])), "written in front of P"
    assert np.array_equal(bits(h[case.off + case.B * case.ld:]), bits(flat[case.off + case.B * case.ld:])), "written past row B"
    assert np.array_equal(bits(body[:, case.N:]), bits(P[:, case.N:])), "the padding [N, ld) changed"
    got = body[:, :case.N]
    same = bits(got) == bits(ref)
    if not same.all():
        d, j = np.argwhere(~same)[0]
        raise AssertionError(f"{int((~same).sum())} of {ref.size} elements differ; first at ({d}, {j}): score {P[d, j]!r} "
                             f"(positive: {bool(pos[d, j])}), got {got[d, j]!r}, expected {ref[d, j]!r}")


def test_grad_of_a_positive_whose_score_equals_dt(lib):
    """include/rtucker_hip.h: only a score of exactly 1.0f or 0.0f is saturated; p == dt gives (p - t0 - dt) s = -t0 s."""
    N, B, eps = 8, 1, 0.1
    t0, dt = bc.constants(N, eps)
    P = np.full((B, N), 0.25, dtype=np.float32)
    P[0, 3] = dt
    Pd, g = dev(P), dev(np.array([bc.GRAD_G], dtype=np.float32))
    slot, ptr, obj = dev(np.zeros(1, np.int64)), dev(np.array([0, 1], np.int64)), dev(np.array([3], np.int64))
    assert lib.rtk_bce_grad_f32(Pd.data_ptr(), B, N, N, slot.data_ptr(), ptr.data_ptr(), obj.data_ptr(), eps, g.data_ptr(),
                                1.0 / (B * N), _stream()) == 0
    torch.cuda.synchronize()
    s = bc.grad_factor(bc.GRAD_G, 1.0 / (B * N))
    got = Pd.cpu().numpy()
    assert bits(got[0, 3]) == bits(-t0 * s), (got[0, 3], -t0 * s)
    assert np.all(bits(got[0, [0, 1, 2, 4, 5, 6, 7]]) == bits((np.float32(0.25) - t0) * s))


# ---------------------------------------------------------------------------------------------- patch -----
@pytest.mark.parametrize("case", bc.PATCH_CASES, ids=lambda c: c.name)
def test_patch_positions_bits_and_row_corrections(lib, case):
    csr, X, v, O, z = bc.patch_operands(case)
    ref_x, ref_c, bound = bc.patch_reference(case, csr, X, z)
    slot, ptr, obj = csr_dev(csr)
    Xd, vd, Od = dev(X), dev(v), dev(O)
    rows_pos = torch.full((4 * case.B + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.rtk_bce_patch_pos_f32(Xd.data_ptr(), case.B, case.N, case.N + case.pad, slot.data_ptr(), ptr.data_ptr(),
                                   obj.data_ptr(), case.eps, vd.data_ptr(), Od.data_ptr(), case.c, rows_pos.data_ptr(),
                                   _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    r = rows_pos.cpu().numpy()
    assert np.isnan(r[4 * case.B:]).all() and np.isfinite(r[:4 * case.B]).all()
    got_x = Xd.cpu().numpy()
    same = bits(got_x) == bits(ref_x)
    assert same.all(), f"X differs at {np.argwhere(~same)[:4].tolist()} (padding, a zero, a non-positive or x - dt)"
    got_c = r[:4 * case.B].reshape(case.B, 4).sum(axis=1)
    err = np.abs(got_c - ref_c)
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print(f"\n[bce patch] {case.name}: max error / bound = {ratio:.4f}")
    assert np.all(err <= bound), f"row {int(np.argmax(err - bound))}: got {got_c[np.argmax(err - bound)]!r}, " \
                                 f"expected {ref_c[np.argmax(err - bound)]!r}"


# ---------------------------------------------------------------------------------------------- fused -----
def _pack(lib, v):
    B, c = v.shape
    vd = dev(v)
    qp = torch.empty(lib.rtk_packed_query_bytes(0, B, c), dtype=torch.uint8, device="cuda")
    assert lib.rtk_pack_query_vectors(vd.data_ptr(), B, c, 0, qp.data_ptr(), _stream()) == 0, lib.rtk_last_error_string()
    return qp


@pytest.mark.parametrize("case", bc.FUSED_CASES, ids=lambda c: c.name)
def test_fused_epilogue_against_the_score_kernel(lib, case):
    B, N, c, ld = case.B, case.N, case.c, case.N + case.pad
    v, O = bc.fused_operands(case)
    qp, Od = _pack(lib, v), dev(O)
    Pd = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.rtk_score_packed_f32(qp.data_ptr(), B, c, Od.data_ptr(), N, Pd.data_ptr(), ld,
                                  SIGMOID | SIGMOID_FAST | KERNEL_V3, _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    Pfull = Pd.cpu().numpy()
    P = Pfull[:, :N]
    nan_bits = bits(np.full(1, np.nan, np.float32))[0]
    assert np.all(bits(Pfull[:, N:]) == nan_bits) and np.isfinite(P).all() and P.min() >= 0 and P.max() <= 1
    if case.scale >= 40 and B * N >= 1000:
        assert (P == 1.0).any() and (P == 0.0).any(), "both saturations must occur"
    eps = case.eps
    if case.find_eps:
        found = bc.find_eps_for(P, N)
        assert found is not None, "no stored p below 1 / N is float32(eps) / float32(N) for a float32 eps"
        eps = found[0]
    t0 = bc.constants(N, eps)[0]
    n_part = lib.rtk_score_bce_partials()
    assert n_part == 512
    Xd = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    partials = torch.full((n_part + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.rtk_score_packed_bce_f32(qp.data_ptr(), B, c, Od.data_ptr(), N, Xd.data_ptr(), ld, eps, partials.data_ptr(),
                                      _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    Xfull, part = Xd.cpu().numpy(), partials.cpu().numpy()
    assert np.all(bits(Xfull[:, N:]) == nan_bits), "the padding [N, ld) was written"
    assert np.isnan(part[n_part:]).all() and np.isfinite(part[:n_part]).all()
    ref_x = bc.fused_x_reference(P, t0)
    same = bits(Xfull[:, :N]) == bits(ref_x)
    if not same.all():
        d, j = np.argwhere(~same)[0]
        raise AssertionError(f"{int((~same).sum())} of {same.size} stored values differ; first at ({d}, {j}): p = {P[d, j]!r}, "
                             f"got {Xfull[d, j]!r}, expected {ref_x[d, j]!r}")
    if case.find_eps:
        assert (P == t0).any() and (bits(Xfull[:, :N]) == 1).any(), "the x == 0 -> smallest denormal branch was not reached"
    ref, mag = bc.negatives_reference(P, N, eps)
    bound = 32 * bc.U * mag + B * N * 2.0 ** -23
    err = abs(float(part[:n_part].sum()) - ref)
    print(f"\n[bce fused] {case.name}: eps = {eps!r}, saturated 1.0f / 0.0f: {int((P == 1).sum())} / {int((P == 0).sum())}, "
          f"subnormal p: {int(((P > 0) & (P < 2.0 ** -126)).sum())}, error / bound = {err / bound:.4f}")
    assert err <= bound, (float(part[:n_part].sum()), ref)


# ---------------------------------------------------------------------------------------------- refusals --
def test_refusals_without_a_launch(lib):
    N, B, c = 16, 4, 8
    P = dev(np.full((B, N), 0.25, np.float32))
    slot, ptr, obj = dev(np.zeros(B, np.int64)), dev(np.array([0, 1], np.int64)), dev(np.array([3], np.int64))
    rows = torch.full((4 * B,), -7.0, dtype=torch.float64, device="cuda")
    g = dev(np.array([1.0], np.float32))
    v, O = dev(np.ones((B, c), np.float32)), dev(np.ones((N, c), np.float32))
    qp = _pack(lib, np.ones((B, c), np.float32))
    part = torch.full((512,), -7.0, dtype=torch.float64, device="cuda")
    p, s, pt, ob, r, st = P.data_ptr(), slot.data_ptr(), ptr.data_ptr(), obj.data_ptr(), rows.data_ptr(), _stream()

    def rows_f(P=p, B=B, N=N, ld=N, s=s, pt=pt, ob=ob, eps=0.1, r=r):
        return lib.rtk_bce_rows_f32(P, B, N, ld, s, pt, ob, eps, r, st)

    def grad_f(P=p, B=B, N=N, ld=N, s=s, pt=pt, ob=ob, eps=0.1, g=g.data_ptr()):
        return lib.rtk_bce_grad_f32(P, B, N, ld, s, pt, ob, eps, g, 1.0, st)

    def patch_f(P=p, B=B, N=N, ld=N, s=s, pt=pt, ob=ob, eps=0.1, v=v.data_ptr(), O=O.data_ptr(), c=c, r=r):
        return lib.rtk_bce_patch_pos_f32(P, B, N, ld, s, pt, ob, eps, v, O, c, r, st)

    def fused_f(q=qp.data_ptr(), B=B, c=c, O=O.data_ptr(), N=N, X=p, ld=N, eps=0.1, part=part.data_ptr()):
        return lib.rtk_score_packed_bce_f32(q, B, c, O, N, X, ld, eps, part, st)

    for f in (rows_f, grad_f, patch_f, fused_f):
        assert f(eps=1.0) == RTK_ERR_BAD_ARG and f(eps=-0.5) == RTK_ERR_BAD_ARG
        assert f(ld=N - 1) == RTK_ERR_BAD_ARG
        assert f(B=0) == RTK_ERR_BAD_ARG and f(N=0) == RTK_ERR_BAD_ARG
    for f in (rows_f, grad_f, patch_f):
        for name in ("P", "s", "pt", "ob"):
            assert f(**{name: None}) == RTK_ERR_BAD_ARG, name
    assert rows_f(r=None) == RTK_ERR_BAD_ARG and grad_f(g=None) == RTK_ERR_BAD_ARG
    for name in ("v", "O", "r"):
        assert patch_f(**{name: None}) == RTK_ERR_BAD_ARG
    assert patch_f(c=0) == RTK_ERR_BAD_ARG
    for name in ("q", "O", "X", "part"):
        assert fused_f(**{name: None}) == RTK_ERR_BAD_ARG
    assert grad_f(B=65536) == RTK_ERR_UNSUPPORTED
    assert fused_f(c=513) == RTK_ERR_UNSUPPORTED
    assert b"513" in lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert torch.all(P == 0.25) and torch.all(rows == -7.0) and torch.all(part == -7.0)
    assert rows_f() == 0 and fused_f() == 0                   # and the plain calls are taken
    torch.cuda.synchronize()
