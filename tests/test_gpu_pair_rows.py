"""GPU tests of rtk_pair_rows_f32 (csrc/rtk_pair_bwd.hip): the row gradients of relation prediction,

    rows[d, j] = sum_i w[d, i] * sum_k core[i, j, k] X[x_idx[d], k]

against the float64 model within its bound (tests/relation_grad_model.py: the forward's own bound with a and b
exchanged), through the ctypes ABI with pitched w and rows and a workspace tail, on the smallest shapes at which each
mechanism of the kernel can go wrong; and the bits of a row: they depend on the query alone."""
import numpy as np
import pytest
import torch

import relation_grad_model as gm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rows_abi(rt, core, X, idx, w, pad=3):
    """rtk_pair_rows_f32 on host arrays -> rows (B, b) on the host.  w has a pitch of a + pad, rows one of b + pad and the
    workspace a tail behind the queried size, all filled with sentinels that must survive; the error word must stay 0."""
    lib = rt._lib.load()
    a, b, c = core.shape
    B = w.shape[0]
    need = lib.rtk_pair_rows_workspace_bytes(B, a, b, c)
    assert need > 0
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    ws[:256].zero_()
    wd = torch.full((B, a + pad), 1e30, dtype=torch.float32, device="cuda")
    wd[:, :a] = _dev(w)
    rows = torch.full((B, b + pad), -7.0, dtype=torch.float32, device="cuda")
    G, Xd, xi = _dev(core), _dev(X), _dev(idx)
    rt._lib.check(lib.rtk_pair_rows_f32(G.data_ptr(), a, b, c, Xd.data_ptr(), Xd.shape[0], xi.data_ptr(), wd.data_ptr(), a + pad,
                                        B, rows.data_ptr(), b + pad, ws.data_ptr(), need,
                                        torch.cuda.current_stream().cuda_stream), "rtk_pair_rows_f32")
    torch.cuda.synchronize()
    assert torch.all(ws[need:] == 0x5A), "wrote past the workspace"
    assert torch.all(rows[:, b:] == -7.0), "wrote past a row"
    assert torch.all(wd[:, a:] == 1e30)
    assert int(ws[:4].view(torch.int32).item()) == 0
    return rows[:, :b].cpu().numpy()


CASES = [
    (1, 1, 4, 1),            # smallest shape
    (3, 5, 4, 33),           # a < 32, two query tiles
    (10, 36, 36, 70),        # a < 32, KS 3
    (40, 36, 36, 33),        # a % 32 != 0, two chunks per j
    (64, 8, 16, 5),          # two full chunks
    (10, 200, 200, 70),      # the WN18RR rank
    (7, 32, 16, 300),        # few tiles, many query tiles: qsplit > 1
    (32, 2080, 4, 33),       # more than 512 row tiles: a workgroup takes several
    (2, 208, 208, 40),       # KS 13
    (5, 24, 52, 40),         # b != c
]


@pytest.mark.parametrize("shape", CASES, ids=["x".join(map(str, s)) for s in CASES])
def test_rows_against_float64(rt, shape):
    a, b, c, B = shape
    core, X, idx, w = gm.rows_case(a, b, c, B)
    want, tau = gm.rows_bounds(core, X, idx, w)
    got = _rows_abi(rt, core, X, idx, w)
    assert np.all(np.isfinite(got))
    ratio = np.max(np.abs(got - want) / np.maximum(tau, 1e-300))
    print(f"a={a} b={b} c={c} B={B}: max |d rows| / tau = {ratio:.2e}")
    assert np.all(np.abs(got - want) <= tau), f"max |d rows| / tau = {ratio:.3e}"


@pytest.mark.parametrize("rank,B", [((10, 36, 36), 70), ((40, 32, 32), 300)])
def test_rows_do_not_depend_on_the_batch(rt, rank, B):
    """bit for bit: the same queries permuted, the first 33 alone (another grid), three queries each alone, a second run."""
    a, b, c = rank
    core, X, idx, w = gm.rows_case(a, b, c, B, seed=3)
    G, Xd, xi, wd = _dev(core), _dev(X), _dev(idx), _dev(w)
    rows = rt.pair_rows(G, Xd, xi, wd)
    assert rows.shape == (B, b) and rows.dtype == torch.float32
    assert torch.equal(rows, rt.pair_rows(G, Xd, xi, wd))
    perm = torch.from_numpy(np.random.default_rng(1).permutation(B)).cuda()
    assert torch.equal(rt.pair_rows(G, Xd, xi[perm], wd[perm]), rows[perm])
    assert torch.equal(rt.pair_rows(G, Xd, xi[:33], wd[:33]), rows[:33])
    for d in (0, 31, B - 1):
        assert torch.equal(rt.pair_rows(G, Xd, xi[d:d + 1], wd[d:d + 1]), rows[d:d + 1])
    want, tau = gm.rows_bounds(core, X, idx, w)
    assert np.all(np.abs(rows.cpu().numpy() - want) <= tau)
    assert rt.pair_rows(G, Xd, xi[:0], wd[:0]).shape == (0, b)


def test_out_of_range_ids(rt):
    """An id outside the table raises IndexError under "strict" and at check_device_errors() under "deferred"; the id is
    clamped and the other rows of the batch keep their bits."""
    a, b, c, B = 5, 36, 36, 40
    core, X, idx, w = gm.rows_case(a, b, c, B, seed=5)
    G, Xd, xi, wd = _dev(core), _dev(X), _dev(idx), _dev(w)
    good = rt.pair_rows(G, Xd, xi, wd)
    for bad in (X.shape[0], -1, X.shape[0] + 7):
        x2 = xi.clone()
        x2[17] = bad
        with rt.index_check("strict"):
            with pytest.raises(IndexError, match="object_idx"):
                rt.pair_rows(G, Xd, x2, wd)
        with rt.index_check("deferred"):
            rows = rt.pair_rows(G, Xd, x2, wd)
            keep = torch.arange(B, device="cuda") != 17
            assert torch.equal(rows[keep], good[keep]) and torch.isfinite(rows[17]).all()
            with pytest.raises(IndexError, match="object_idx"):
                rt.check_device_errors()
        rt.check_device_errors()                                        # the word was cleared
