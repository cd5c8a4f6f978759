"""The host-level paths that reach the exact-fp32 GEMM and the stage-1 backward, and the logistic's derivative.

  * rtk_sigmoid_grad_f32 / rtk_sigmoid_grad_rows_f32 against float64, element by element;
  * score_1vN(sigmoid=False).backward with integer operands and an integer upstream gradient: the saved query
    vectors and all four gradients bit for bit against float64, for both backward GEMMs;
  * one backward at B = 65 537: the dense rtk_sigmoid_grad_f32 branch of _Score1vN.backward (B > 65535) together
    with the scatter that reads its ids from global memory (B > 8192).
"""
import numpy as np
import pytest
import torch

import exact_cases as ec
from oracle import score_oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
U = 2.0 ** -24
DENORMAL_FLOOR = 2.0 ** -149


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ dZ = dP * P * (1 - P) ----------------
def _sigmoid_grad_inputs(n, seed):
    rng = np.random.default_rng(seed)
    P = (1.0 / (1.0 + np.exp(-rng.normal(0, 4, n)))).astype(np.float32)       # saturates to exactly 0 / 1 in places
    P[::97] = 1.0
    P[5::101] = 0.0
    P[7::103] = np.float32(2.0 ** -24)
    dP = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 0, n))).astype(np.float32)
    dP[3::89] = np.float32(1e-30)
    return dP, P


def _sigmoid_grad_check(got, dP, P):
    """The kernel rounds four times at most (1 - p, two products, the store): |err| <= 4 u |ref| + denormal floor."""
    ref = dP.astype(np.float64) * P.astype(np.float64) * (1.0 - P.astype(np.float64))
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= 4 * U * np.abs(ref) + DENORMAL_FLOOR), float(np.max(err / (4 * U * np.abs(ref) + DENORMAL_FLOOR)))


@pytest.mark.parametrize("n,off", [(1, 0), (3, 0), (4099, 0), (4096, 1), (65537 * 3, 0), (1031, 1)])
@pytest.mark.parametrize("alias", [False, True])
def test_sigmoid_grad_contiguous(rt, n, off, alias):
    """n % 4 != 0 (the scalar tail), every pointer one float off a 16-byte boundary (the scalar path), dZ aliasing dP."""
    lib = rt._lib.load()
    dP, P = _sigmoid_grad_inputs(n, n + off)
    pad = lambda x: torch.from_numpy(np.concatenate([np.full(off, SENTINEL, np.float32), x, np.full(8, SENTINEL, np.float32)])).cuda()  # noqa: E731
    tg, tp = pad(dP), pad(P)
    tz = tg if alias else torch.full_like(tg, SENTINEL)
    rc = lib.rtk_sigmoid_grad_f32(tg.data_ptr() + 4 * off, tp.data_ptr() + 4 * off, tz.data_ptr() + 4 * off, n, _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    z = tz.cpu().numpy()
    assert np.all(z[:off] == SENTINEL) and np.all(z[off + n:] == SENTINEL)
    assert np.array_equal(tp.cpu().numpy()[off:off + n], P)                    # P is only read
    _sigmoid_grad_check(z[off:off + n], dP, P)


@pytest.mark.parametrize("batch,n,lds", [(5, 1031, (1031, 1040, 1056)), (1, 7, (9, 7, 8)), (300, 257, (288, 257, 261)),
                                         (2, 4100, (4100, 4128, 4101))])
def test_sigmoid_grad_rows(rt, batch, n, lds):
    """Three different pitches (dP, P, dZ); the padding of dZ keeps its sentinel."""
    lib = rt._lib.load()
    dP, P = _sigmoid_grad_inputs(batch * n, n)
    ld_g, ld_p, ld_z = lds

    def pitched(x, ld):
        st = np.full((batch, ld), SENTINEL, np.float32)
        st[:, :n] = x.reshape(batch, n)
        return torch.from_numpy(st).cuda()
    tg, tp = pitched(dP, ld_g), pitched(P, ld_p)
    tz = torch.full((batch, ld_z), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.rtk_sigmoid_grad_rows_f32(tg.data_ptr(), ld_g, tp.data_ptr(), ld_p, tz.data_ptr(), ld_z, batch, n, _stream())
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    z = tz.cpu().numpy()
    assert np.all(z[:, n:] == SENTINEL)
    _sigmoid_grad_check(z[:, :n].reshape(-1), dP, P)
    # a pitch below n and a batch beyond the grid limit are refused, nothing written
    tz.fill_(SENTINEL)
    assert lib.rtk_sigmoid_grad_rows_f32(tg.data_ptr(), ld_g, tp.data_ptr(), ld_p, tz.data_ptr(), n - 1, batch, n, _stream()) == -1
    assert lib.rtk_sigmoid_grad_rows_f32(tg.data_ptr(), ld_g, tp.data_ptr(), ld_p, tz.data_ptr(), ld_z, 65536, n, _stream()) == -3
    torch.cuda.synchronize()
    assert torch.all(tz == SENTINEL)


# ------------------------------------------------------------------ integer backward through score_1vN ----
def integer_model(B, N, n_rel, n_sub, rank, nz, seed):
    """Integer-valued operands and an integer upstream gradient for which no step of the backward can round:
    core sparse signs, R and S in {-1, 0, 1}, O odd integers of exactly 12 significant bits, the upstream gradient
    with `nz` entries of +-1 per query.  Every abs-sum (v, g_O, dv and the three stage-1 gradients) is asserted
    below 2^24."""
    rng = np.random.default_rng(seed)
    a, b, c = rank
    core = ec.signs(rng, (a, b, c), 0.25)
    R, S = ec.signs(rng, (n_rel, a), 0.7), ec.signs(rng, (n_sub, b), 0.7)
    O = ec.wide_ints(rng, (N, c), 12)
    h, r = rng.integers(0, n_sub, B), rng.integers(0, n_rel, B)
    dZ = np.zeros((B, N), dtype=np.float32)
    for d in range(B):
        dZ[d, rng.choice(N, size=min(nz, N), replace=False)] = rng.choice([-1.0, 1.0], size=min(nz, N))
    f8 = lambda x: np.abs(x).astype(np.float64)  # noqa: E731
    v_abs = np.einsum("abc,da,db->dc", f8(core), f8(R)[r], f8(S)[h])
    dv_abs = f8(dZ) @ f8(O)
    sums = [v_abs, f8(dZ).T @ v_abs, dv_abs, *ec.bwd_ref(f8(core), f8(R), f8(S), dv_abs, r, h)]
    assert max(float(x.max()) for x in sums) < ec.LIMIT, [float(x.max()) for x in sums]
    assert v_abs.max() < 2 ** 11        # what the split-fp16 argument needs of v: hi + lo hold it without loss
    return core, R, S, O, h, r, dZ


@pytest.mark.parametrize("mode", ["split_fp16", "f32"])
@pytest.mark.parametrize("B,N,nz", [(1, 37, 3), (130, 515, 3), (200, 1031, 3)])
def test_score_1vN_integer_backward_bit_exact(rt, mode, B, N, nz):
    """score_1vN(sigmoid=False): logits, so the upstream gradient IS dZ.  Relation rank 4 <= 32: stage 1 is the VALU
    path.  First the saved device query vectors equal the exact integer v (a forward check in its own right), then
    g_O = dZ^T v, g_core, g_R and g_S equal float64 bit for bit.  B = 1 is the `ld` special case of the pitch
    arguments; N = 515 and 1031 are dense odd entity counts; at N = 1031 _splits_for(B, c, N) = 2, so dv = dZ O
    is a two-slab split-K product (the split factor grows with K = N, not with B).

    Why the split-fp16 GEMM is exact here too: each operand is scaled by a power of two (exact); the wide operand
    (O: 12 bits; v: integers below 2^11) fits hi + lo = 22 bits, so its split loses nothing; the other operand
    (dZ in {-1, 0, 1}) has a zero lo half, so the dropped lo.lo product is zero; and the fp32 accumulation adds
    integers (times one common power of two) whose abs-sum is below 2^24."""
    rank = (4, 16, 16)                  # (subject rank == object rank, as the reference's .view requires)
    core, R, S, O, h, r, dZ = integer_model(B, N, 40, 300, rank, nz, seed=B + N)
    v_ref = np.einsum("abc,da,db->dc", *[x.astype(np.float64) for x in (core, R[r], S[h])])
    dv_ref = dZ.astype(np.float64) @ O.astype(np.float64)
    gO_ref = dZ.astype(np.float64).T @ v_ref
    gcore_ref, gR_ref, gS_ref = ec.bwd_ref(core, R, S, dv_ref, r, h)
    if N >= 1024:
        assert rt.ops._splits_for(B, rank[2], N) > 1
    rt.ops.BACKWARD_GEMM = mode
    try:
        leaves = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (core, R, S, O)]
        out = rt.score_1vN(*leaves, torch.from_numpy(h).cuda(), torch.from_numpy(r).cuda(), sigmoid=False)
        # (the order of _Score1vN.forward's save_for_backward: core, R, S, O, h, r, v, out -- a private detail of ops.py)
        v_dev = out.grad_fn.saved_tensors[6]
        assert v_dev.shape == (B, rank[2])
        assert np.array_equal(v_dev.cpu().numpy().astype(np.float64), v_ref), "forward query vectors are not the exact integers"
        out.backward(torch.from_numpy(dZ).cuda())
        torch.cuda.synchronize()
    finally:
        rt.ops.BACKWARD_GEMM = "split_fp16"
    for name, leaf, ref in (("g_O", leaves[3], gO_ref), ("g_core", leaves[0], gcore_ref), ("g_R", leaves[1], gR_ref),
                            ("g_S", leaves[2], gS_ref)):
        got = leaf.grad.cpu().numpy()
        bad = np.argwhere(got.astype(np.float64) != ref)
        assert len(bad) == 0, (f"{name} ({mode}): {len(bad)} of {ref.size} differ; first at {tuple(bad[0])}: "
                               f"got {got[tuple(bad[0])]!r}, expected {ref[tuple(bad[0])]!r}")


# ------------------------------------------------------------------ B = 65 537 ---------------------------
def test_backward_at_batch_65537(rt):
    """B > 65535: _Score1vN.backward takes the dense rtk_sigmoid_grad_f32 branch; B > 8192: the scatter reads its ids
    from global memory (lists of ~13 000 queries per relation).  Against float64 autograd through the oracle's op
    sequence, with the tolerance of test_gradients_medium_against_oracle_autograd (2e-4 of max|g|)."""
    n_ent, n_rel, B, rank = 40, 5, 65537, (3, 8, 8)
    rng = np.random.default_rng(65537)
    core, R, S, O = [rng.standard_normal(s).astype(np.float32) * np.float32(0.5)
                     for s in (rank, (n_rel, rank[0]), (n_ent, rank[1]), (n_ent, rank[2]))]
    h, r = rng.integers(0, n_ent, B), rng.integers(0, n_rel, B)
    w = rng.standard_normal((B, n_ent)).astype(np.float32)
    ref = orc.score_grads_ref(*[torch.from_numpy(x).double() for x in (core, R, S, O)], torch.from_numpy(h),
                              torch.from_numpy(r), torch.from_numpy(w).double())
    leaves = [torch.from_numpy(x).cuda().requires_grad_(True) for x in (core, R, S, O)]
    P = rt.score_1vN(*leaves, torch.from_numpy(h).cuda(), torch.from_numpy(r).cuda())
    assert P.shape == (B, n_ent)
    (P * torch.from_numpy(w).cuda()).sum().backward()
    torch.cuda.synchronize()
    for name, leaf, g in zip(("g_core", "g_R", "g_S", "g_O"), leaves, ref):
        scale = g.abs().max().item() + 1e-12
        rel = (leaf.grad.cpu().double() - g).abs().max().item() / scale
        print(f"\n[B = 65537] {name}: max |err| / max|g| = {rel:.3e}")
        assert rel < 2e-4, name
