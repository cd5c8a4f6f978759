"""GPU tests of rtk_scatter_rows_f32 (csrc/rtk_pair_bwd.hip): out[e, :] = sum_{d: idx[d] = e} rows[d, :], the ordered
scatter with one entry per query.  Against float64 within (m + 2) 2^-24 sum |rows| over the m queries that name a row
(tests/relation_grad_model.py); rows nobody names are zero, ids outside the table add nothing, two runs give equal
bits."""
import numpy as np
import pytest
import torch

import relation_grad_model as gm

pytestmark = pytest.mark.gpu

N_OUT = 60


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _ids(kind, B, rng):
    if kind == "one":
        return np.full(B, 7, dtype=np.int64)
    if kind == "distinct":
        return rng.permutation(max(B, N_OUT))[:B].astype(np.int64)
    idx = rng.integers(0, N_OUT // 4, B).astype(np.int64)                 # "mixed": repeats, and ids outside the table
    idx[::5] = N_OUT + rng.integers(0, 3, idx[::5].shape)
    idx[1::7] = -1 - rng.integers(0, 3, idx[1::7].shape)
    return idx


@pytest.mark.parametrize("n", [1, 36, 200, 1024])
@pytest.mark.parametrize("kind,B", [("one", 300), ("distinct", 50), ("mixed", 700), ("mixed", 1)])
def test_scatter_against_float64(rt, kind, B, n):
    rng = np.random.default_rng(13 * n + B)
    n_out = max(B, N_OUT) if kind == "distinct" else N_OUT
    idx = _ids(kind, B, rng)
    rows = rng.standard_normal((B, n)).astype(np.float32)
    buf = torch.full((B, n + 3), 1e30, dtype=torch.float32, device="cuda")     # pitched rows, the padding never read
    buf[:, :n] = torch.from_numpy(rows).cuda()
    got = rt.scatter_rows(torch.from_numpy(idx).cuda(), buf[:, :n], n_out)
    assert got.shape == (n_out, n) and got.dtype == torch.float32
    assert torch.equal(got, rt.scatter_rows(torch.from_numpy(idx).cuda(), buf[:, :n], n_out))
    assert torch.equal(got, rt.scatter_rows(torch.from_numpy(idx).cuda(), torch.from_numpy(rows).cuda(), n_out))
    want, tau = gm.scatter_rows(idx, rows, n_out)
    err = np.abs(got.cpu().numpy() - want)
    print(f"{kind} B={B} n={n}: max |d out| / tau = {np.max(err / np.maximum(tau, 1e-300)):.2e}")
    assert np.all(err <= tau)
    named = np.zeros(n_out, dtype=bool)
    named[idx[(idx >= 0) & (idx < n_out)]] = True
    assert torch.all(got[torch.from_numpy(~named).cuda()] == 0)


def test_batch_zero_gives_zeros(rt):
    out = rt.scatter_rows(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros((0, 36), device="cuda"), N_OUT)
    assert out.shape == (N_OUT, 36) and torch.all(out == 0)
