"""GPU tests of rtk_core_outer_f32 (csrc/rtk_pair_bwd.hip): gG[i, j, k] = sum_d (x[d, i] * y[d, j]) * z[d, k].

One accumulation chain per element over d ascending, so the bits are those of rtk_gemm_f32 on the materialised left
operand X[d, i b + j] = x[d, i] * y[d, j] (torch.equal), whatever the tile shape; and the float64 bound of one fp32 chain
of B terms holds (tests/relation_grad_model.py)."""
import numpy as np
import pytest
import torch

import relation_grad_model as gm
import relation_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _pitched(x, pad, fill):
    """(view of the values, whole buffer) with a row pitch of width + pad, the padding holding ``fill``."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf[:, :x.shape[1]], buf


def _gemm_reference(rt, x, y, z):
    """rtk_gemm_f32 on the materialised X (B, a*b): M-major X and z, M = a*b, N = c, K = B."""
    lib = rt._lib.load()
    B, a, b, c = x.shape[0], x.shape[1], y.shape[1], z.shape[1]
    X = (x.contiguous()[:, :, None] * y.contiguous()[:, None, :]).reshape(B, a * b).contiguous()     # one fp32 product each
    zc = z.contiguous()
    out = torch.empty((a * b, c), dtype=torch.float32, device="cuda")
    rt._lib.check(lib.rtk_gemm_f32(X.data_ptr(), 0, a * b, zc.data_ptr(), 0, c, out.data_ptr(), c, a * b, c, B, 0,
                                   torch.cuda.current_stream().cuda_stream), "rtk_gemm_f32")
    return out.view(a, b, c)


CASES = [(1, 1, 4, 1), (3, 5, 4, 33), (10, 36, 36, 70), (2, 160, 64, 5), (1, 130, 132, 17), (10, 200, 200, 64)]


@pytest.mark.parametrize("shape", CASES, ids=["x".join(map(str, s)) for s in CASES])
def test_bits_of_the_gemm_and_float64_bound(rt, shape):
    a, b, c, B = shape
    x, y, z = rm.scaled((B, a), 3 * a + B, -3, 3), rm.scaled((B, b), 5 * b + B, -3, 3), rm.scaled((B, c), 7 * c + B, -3, 3)
    (xd, xb), (yd, yb), (zd, zb) = _pitched(x, 3, 1e30), _pitched(y, 1, 1e30), _pitched(z, 3, 1e30)
    got = rt.core_outer(xd, yd, zd)
    torch.cuda.synchronize()
    assert got.shape == (a, b, c) and got.dtype == torch.float32
    assert torch.all(xb[:, a:] == 1e30) and torch.all(yb[:, b:] == 1e30) and torch.all(zb[:, c:] == 1e30)
    assert torch.equal(got, _gemm_reference(rt, xd, yd, zd))
    assert torch.equal(got, rt.core_outer(xd.contiguous(), yd.contiguous(), zd.contiguous()))      # dense, vector loads of z
    want, tau = gm.core_outer(x, y, z), gm.core_outer_bound(x, y, z)
    err = np.abs(got.cpu().numpy() - want)
    print(f"a={a} b={b} c={c} B={B}: max |d gG| / tau = {np.max(err / np.maximum(tau, 1e-300)):.2e}")
    assert np.all(err <= tau)


def test_output_is_written_inside_its_bounds_and_batch_zero_gives_zeros(rt):
    lib = rt._lib.load()
    a, b, c, B = 3, 5, 4, 33
    x, y, z = [torch.from_numpy(rm.scaled((B, n), n)).cuda() for n in (a, b, c)]
    buf = torch.full((a * b * c + 64,), -7.0, dtype=torch.float32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    rt._lib.check(lib.rtk_core_outer_f32(x.data_ptr(), a, a, y.data_ptr(), b, b, z.data_ptr(), c, c, B, buf.data_ptr(), sp),
                  "rtk_core_outer_f32")
    torch.cuda.synchronize()
    assert torch.all(buf[a * b * c:] == -7.0)
    assert torch.equal(buf[:a * b * c].view(a, b, c), rt.core_outer(x, y, z))
    rt._lib.check(lib.rtk_core_outer_f32(None, a, a, None, b, b, None, c, c, 0, buf.data_ptr(), sp), "rtk_core_outer_f32")
    torch.cuda.synchronize()
    assert torch.all(buf[:a * b * c] == 0) and torch.all(buf[a * b * c:] == -7.0)
    assert torch.all(rt.core_outer(x[:0], y[:0], z[:0]) == 0)
