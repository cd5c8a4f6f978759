"""The softmax cross-entropy loss kernels through their four C entry points, on inputs built here: rtk_ce_rows_f32 and
rtk_ce_grad_f32 on planted logit rows, rtk_ce_stream_rows_f32 and rtk_ce_stream_grad_f32 on planes packed from a given
v (rtk_pack_query_vectors).  No stage 1 and no GEMM enters any bound.

Cases, float64 references and the derived bounds: tests/golden/ce_kernel_cases.py (proved on the host by
tests/test_ce_kernel_cases_host.py, mutants included).  Every result is held to its bound per element; the largest
error / bound of every case is printed.  Guards behind every output are NaN before and afterwards, row padding
(ld > N) keeps its bits, a second run gives the same bits.
"""
import functools

import numpy as np
import pytest
import torch

import ce_kernel_cases as cc

pytestmark = pytest.mark.gpu

GUARD = 64
by_name = dict(ids=lambda c: c.name)


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


def csr_ptrs(csr):
    keep = dev(csr.slot), dev(csr.ptr), dev(csr.obj)
    return keep, [t.data_ptr() for t in keep]


def nan_buf(n, dtype):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")


# ---------------------------------------------------------------------------------------------- matrix form
def run_rows(lib, case, Zd, csr_p):
    rows, lse = nan_buf(case.B, torch.float64), nan_buf(case.B, torch.float32)
    rc = lib.rtk_ce_rows_f32(Zd.data_ptr(), case.B, case.N, case.ld, *csr_p, case.eps, rows.data_ptr(), lse.data_ptr(),
                             _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    return rows.cpu().numpy(), lse.cpu().numpy()


@pytest.mark.parametrize("case", cc.ROWS_CASES, **by_name)
def test_rows_against_float64(lib, case):
    csr, Z = cc.setup_rows(case)
    keep, csr_p = csr_ptrs(csr)
    Zd = dev(Z)
    rows, lse = run_rows(lib, case, Zd, csr_p)
    rows2, lse2 = run_rows(lib, case, Zd, csr_p)
    assert np.array_equal(rows.view(np.uint64), rows2.view(np.uint64)) and np.array_equal(bits(lse), bits(lse2)), \
        "second run differs in its bits"
    assert np.isnan(rows[case.B:]).all() and np.isnan(lse[case.B:]).all(), "written past row B"
    assert np.array_equal(bits(Zd.cpu().numpy()), bits(Z)), "Z was written"
    r_lse, r_rows = cc.rows_verdict(case, Z, csr, lse[:case.B], rows[:case.B])
    print(f"\n[ce rows] {case.name}: max error / bound = {r_lse:.4f} (lse_out), {r_rows:.4f} (rows_out)")
    assert r_lse <= 1.0 and r_rows <= 1.0


def run_grad(lib, case, Z, csr_p, lse32):
    """-> the (B, ld) block afterwards; checks the bytes in front of it and behind it."""
    g = dev(np.array([cc.GRAD_G], dtype=np.float32))
    flat = np.concatenate([np.full(case.off, np.nan, np.float32), Z.reshape(-1), np.full(GUARD, np.nan, np.float32)])
    buf, lse_d = dev(flat), dev(lse32)
    z_ptr = buf.data_ptr() + 4 * case.off
    assert ((case.ld % 4 == 0) and z_ptr % 16 == 0) == (case.ld % 4 == 0 and case.off % 4 == 0)
    rc = lib.rtk_ce_grad_f32(z_ptr, case.B, case.N, case.ld, *csr_p, case.eps, lse_d.data_ptr(), g.data_ptr(),
                             float(cc.grad_scale(case)), _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    end = case.off + case.B * case.ld
    assert np.array_equal(bits(h[:case.off]), bits(flat[:case.off])), "written in front of Z"
    assert np.array_equal(bits(h[end:]), bits(flat[end:])), "written past row B"
    return h[case.off:end].reshape(case.B, case.ld)


@pytest.mark.parametrize("case", cc.GRAD_CASES, **by_name)
def test_grad_against_float64(lib, case):
    csr, Z = cc.setup_rows(case)
    keep, csr_p = csr_ptrs(csr)
    lse32 = cc.rows_reference(case, Z, csr)[0].astype(np.float32)
    body = run_grad(lib, case, Z, csr_p, lse32)
    assert np.array_equal(bits(body[:, case.N:]), bits(Z[:, case.N:])), "the padding [N, ld) changed"
    r = cc.grad_verdict(case, Z, csr, lse32, body)
    print(f"\n[ce grad] {case.name}: max error / bound = {r:.4f}")
    assert r <= 1.0


def test_grad_chained_to_the_rows_kernel(lib):
    """rtk_ce_rows_f32's own lse_out into the gradient: every element within its bound for that lse, and each row sums
    to (w_d - the mass of its in-range targets) s within the summed bounds plus w |s| times the bound of lse_out."""
    case = cc.CHAINED_CASE
    csr, Z = cc.setup_rows(case)
    keep, csr_p = csr_ptrs(csr)
    _, lse = run_rows(lib, case, dev(Z), csr_p)
    lse = lse[:case.B].copy()
    body = run_grad(lib, case, Z, csr_p, lse)
    r = cc.grad_verdict(case, Z, csr, lse, body)
    ref = cc.grad_reference(case, Z, csr, lse)
    bound = cc.grad_bound(case, Z, csr, lse, ref).sum(axis=1)
    t0, dt, eps = cc.consts32(case.N, case.eps)
    s = float(np.float32(cc.GRAD_G) * cc.grad_scale(case))
    n = csr.stored()
    w = cc.weights(n, dt, eps).astype(np.float64)
    k = np.array([len(csr.positives(d, case.N)) for d in range(case.B)])
    mass = case.N * float(t0) + np.where(n > 0, float(dt) / np.maximum(n, 1) * k, 0.0)
    lse_b = cc.rows_bounds(case, Z, csr)[1]
    bound = bound + 1.01 * w * abs(s) * lse_b
    err = np.abs(body[:, :case.N].astype(np.float64).sum(axis=1) - (w - mass) * s)
    print(f"\n[ce grad] {case.name}: max error / bound = {r:.4f} (elements), {float((err / bound).max()):.4f} (row sums)")
    assert r <= 1.0 and np.all(err <= bound)


# ---------------------------------------------------------------------------------------------- matrix-free
@functools.lru_cache(maxsize=None)
def stream_setup(case):
    data = cc.stream_operands(case)
    fwd = cc.stream_forward(case, data)
    return data, fwd, fwd[0].astype(np.float32)


class Device:
    """The operands of a case on the device: packed planes, O, v, the CSR."""

    def __init__(self, lib, case, data):
        self.case, self.lib = case, lib
        B, c = case.B, case.c
        self.v, self.O = dev(data.v), dev(data.O)
        self.qp = torch.empty(lib.rtk_packed_query_bytes(0, B, c), dtype=torch.uint8, device="cuda")
        assert lib.rtk_pack_query_vectors(self.v.data_ptr(), B, c, 0, self.qp.data_ptr(), _stream()) == 0, \
            lib.rtk_last_error_string()
        self.keep, self.csr_p = csr_ptrs(data.csr)
        self.scale = dev(np.array([cc.stream_scale(case)], dtype=np.float32))

    def workspace(self, max_pos):
        n = self.lib.rtk_ce_stream_workspace_bytes(self.case.B, self.case.N, self.case.c, max_pos)
        assert n > 0
        return torch.zeros(n, dtype=torch.uint8, device="cuda")

    def rows(self):
        case, ws = self.case, self.workspace(0)
        rows, lse = nan_buf(case.B, torch.float64), nan_buf(case.B, torch.float32)
        rc = self.lib.rtk_ce_stream_rows_f32(self.qp.data_ptr(), case.B, case.c, self.O.data_ptr(), case.N, *self.csr_p,
                                             case.eps, rows.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        return rows.cpu().numpy(), lse.cpu().numpy()

    def grad(self, lse32, max_pos, want_dv=True, want_gO=True):
        """-> (dv with its guard, gO with its guard, error word); gO is -7.0 before."""
        case, ws = self.case, self.workspace(max_pos)
        lse_d = dev(lse32)
        dv = nan_buf(case.B * case.c, torch.float32)
        gO = nan_buf(case.N * case.c, torch.float32)
        gO[:case.N * case.c] = -7.0
        rc = self.lib.rtk_ce_stream_grad_f32(self.qp.data_ptr(), self.v.data_ptr(), case.B, case.c, self.O.data_ptr(), case.N,
                                             *self.csr_p, max_pos, case.eps, lse_d.data_ptr(), self.scale.data_ptr(),
                                             dv.data_ptr() if want_dv else None, gO.data_ptr() if want_gO else None,
                                             ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        return dv.cpu().numpy(), gO.cpu().numpy(), int(ws[:4].view(torch.int32).item())


@pytest.mark.parametrize("case", cc.STREAM_CASES, **by_name)
def test_stream_forward_against_float64(lib, case):
    data, fwd, _ = stream_setup(case)
    d = Device(lib, case, data)
    rows, lse = d.rows()
    rows2, lse2 = d.rows()
    assert np.array_equal(rows.view(np.uint64), rows2.view(np.uint64)) and np.array_equal(bits(lse), bits(lse2)), \
        "second run differs in its bits"
    assert np.isnan(rows[case.B:]).all() and np.isnan(lse[case.B:]).all(), "written past row B"
    r_lse, r_rows = cc.stream_forward_verdict(fwd, lse[:case.B], rows[:case.B])
    print(f"\n[ce stream rows] {case.name}: max error / bound = {r_lse:.4f} (lse_out), {r_rows:.4f} (loss_rows_out)")
    assert r_lse <= 1.0 and r_rows <= 1.0


@pytest.mark.parametrize("case", cc.STREAM_CASES, **by_name)
def test_stream_backward_against_float64(lib, case):
    data, _, lse32 = stream_setup(case)
    ref = cc.stream_backward(case, data, lse32)
    d = Device(lib, case, data)
    B, N, c = case.B, case.N, case.c
    entries = int(data.csr.stored().sum())
    dv, gO, err = d.grad(lse32, B * data.csr.longest())
    assert err == 0
    assert np.isnan(dv[B * c:]).all() and np.isnan(gO[N * c:]).all(), "written past an output"
    assert not (gO[:N * c] == -7.0).any(), "gO is not written in full"
    dv2, gO2, err2 = d.grad(lse32, B * data.csr.longest())
    assert err2 == 0 and np.array_equal(bits(dv), bits(dv2)) and np.array_equal(bits(gO), bits(gO2)), \
        "second run differs in its bits"
    dv3, gO3, err3 = d.grad(lse32, entries)
    assert err3 == 0 and np.array_equal(bits(dv), bits(dv3)) and np.array_equal(bits(gO), bits(gO3)), \
        "max_pos = the batch's CSR entries differs from B * longest"
    r_dv, r_gO = cc.stream_backward_verdict(ref, dv[:B * c].reshape(B, c), gO[:N * c].reshape(N, c))
    print(f"\n[ce stream grad] {case.name}: max error / bound = {r_dv:.4f} (dv_out), {r_gO:.4f} (gO_out)")
    assert r_dv <= 1.0 and r_gO <= 1.0


@pytest.mark.parametrize("case", cc.SINGLE_OUTPUT_CASES, **by_name)
def test_stream_single_outputs_give_the_bits_of_both(lib, case):
    data, _, lse32 = stream_setup(case)
    d = Device(lib, case, data)
    B, N, c = case.B, case.N, case.c
    max_pos = B * data.csr.longest()
    dv, gO, err = d.grad(lse32, max_pos)
    dv1, gO1, err1 = d.grad(lse32, max_pos, want_gO=False)
    dv2, gO2, err2 = d.grad(lse32, max_pos, want_dv=False)
    assert err == 0 and err1 == 0 and err2 == 0
    assert np.array_equal(bits(dv1), bits(dv)) and (gO1[:N * c] == -7.0).all()
    assert np.array_equal(bits(gO2), bits(gO)) and np.isnan(dv2).all()
