"""The exact-fp32 MFMA GEMM (csrc/rtk_gemm_f32.hip) through the C ABI, bit for bit against float64.

Operands come from tests/golden/exact_cases.py: integer-valued fp32 whose abs-sums stay below 2^24, so no product,
partial sum, split-K slab or slab add can round and the kernel must return the float64 result exactly, in any
summation order (tests/test_exact_cases_host.py proves that, and that a dropped / doubled / tail-leaked term or a
narrowed operand is visible, on the host).  A smaller real-valued layer is held to the derived element-wise bound
gamma_n * sum|a||b| (n = the chunk's K + splits); its largest error / bound is printed, never asserted against.

Every case: operands laid out with GARBAGE in the row padding and behind the K tail, C pre-filled with a sentinel,
the columns [N, ldc), the floats before a shifted C and everything past row M still the sentinel afterwards, a
second run bit-identical, the split-K workspace pre-filled with 0xFF bytes.
"""
import numpy as np
import pytest
import torch

import exact_cases as ec

pytestmark = pytest.mark.gpu

SENTINEL = -777.25          # not an integer: no exact result equals it
GUARD = 64                  # floats behind C that must keep the sentinel
P_TOL = 3e-6                # the tolerance tests/test_gpu_parity.py states for probabilities; include/rtucker_hip.h
                            # names no figure of its own for the exact logistic
RTK_ERR_WORKSPACE = -2


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def lay_out(X, kmajor, pad, off):
    """Device storage of the logical (rows, K) operand X.  K-major: rows of K + pad floats; M-major: K + 1 rows of
    rows + pad floats, the last one GARBAGE (what a K tail read too far meets).  `off` floats of GARBAGE in front
    move the base off a 16-byte boundary.  -> (tensor kept alive, pointer, leading dimension)."""
    rows, K = X.shape
    if kmajor:
        st = np.full((rows, K + pad), ec.GARBAGE, dtype=np.float32)
        st[:, :K] = X
    else:
        st = np.full((K + 1, rows + pad), ec.GARBAGE, dtype=np.float32)
        st[:K, :rows] = X.T
    flat = np.concatenate([np.full(off, ec.GARBAGE, np.float32), st.reshape(-1), np.full(16, ec.GARBAGE, np.float32)])
    t = torch.from_numpy(flat).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off, st.shape[1]


def new_c(case):
    ldc = case.N + case.ldc_pad
    buf = torch.full((case.c_off + case.M * ldc + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * case.c_off, ldc


def read_c(case, buf, ldc):
    """The M x N result; asserts that everything around it still holds the sentinel."""
    h = buf.cpu().numpy()
    body = h[case.c_off:case.c_off + case.M * ldc].reshape(case.M, ldc)
    assert np.all(h[:case.c_off] == SENTINEL), "written in front of C"
    assert np.all(h[case.c_off + case.M * ldc:] == SENTINEL), "written past row M"
    assert np.all(body[:, case.N:] == SENTINEL), "written in the columns [N, ldc)"
    return body[:, :case.N].copy()


def call(lib, case, pa, lda, pb, ldb, pc, ldc, flags=0, ws=None, ws_bytes=None):
    if case.entry == "score":
        assert case.ak == 1 and case.bk == 1 and lda == case.K and ldb == case.K
        return lib.rtk_score_f32(pa, case.M, case.K, pb, case.N, pc, ldc, flags, _stream())
    if case.splits == 0:
        return lib.rtk_gemm_f32(pa, case.ak, lda, pb, case.bk, ldb, pc, ldc, case.M, case.N, case.K, flags, _stream())
    return lib.rtk_gemm_f32_splitk(pa, case.ak, lda, pb, case.bk, ldb, pc, ldc, case.M, case.N, case.K, case.splits,
                                   ws.data_ptr() if ws is not None else None,
                                   ws.numel() if ws_bytes is None else ws_bytes, _stream())


def workspace(lib, case):
    if case.splits == 0:
        return None
    n = lib.rtk_gemm_f32_splitk_workspace_bytes(case.M, case.N, case.splits)
    assert n >= case.M * case.N * 4 * case.splits
    return torch.full((max(n, 256),), 0xFF, dtype=torch.uint8, device="cuda")      # NaN bit patterns: never read before written


def run_twice(lib, case, A, B, flags=0):
    ta, pa, lda = lay_out(A, case.ak, case.a_pad, case.a_off)
    tb, pb, ldb = lay_out(B, case.bk, case.b_pad, case.b_off)
    outs = []
    for _ in range(2):
        ws = workspace(lib, case)
        buf, pc, ldc = new_c(case)
        rc = call(lib, case, pa, lda, pb, ldb, pc, ldc, flags, ws)
        assert rc == 0, lib.rtk_last_error_string()
        torch.cuda.synchronize()
        outs.append(read_c(case, buf, ldc))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "second run differs in its bits"
    return outs[0], (pa, lda, pb, ldb, ta, tb)


def first_difference(got, ref):
    bad = np.argwhere(got.astype(np.float64) != ref)
    m, n = bad[0]
    return f"{len(bad)} of {ref.size} elements differ; first at ({m}, {n}): got {got[m, n]!r}, expected {ref[m, n]!r}"


@pytest.mark.parametrize("case", [c for c in ec.GEMM_CASES if c.exact], ids=lambda c: c.name)
def test_gemm_bit_exact(lib, case):
    A, B = ec.gemm_operands(case)                    # asserts max abs-sum < 2^24
    ref = ec.gemm_ref(A, B)
    got, _ = run_twice(lib, case, A, B)
    assert np.array_equal(got.astype(np.float64), ref), first_difference(got, ref)


@pytest.mark.parametrize("case", [c for c in ec.GEMM_CASES if not c.exact], ids=lambda c: c.name)
def test_gemm_real_values_within_gamma_bound(lib, case):
    A, B = ec.gemm_operands(case)
    ref, bound = ec.gemm_ref(A, B), ec.gemm_bound(case, A, B)
    got, _ = run_twice(lib, case, A, B)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"\n[gemm real] {case.name}: K = {case.K}, splits = {max(case.splits, 1)}, max error / gamma bound = {ratio:.4f}")
    assert np.isfinite(got).all() and np.all(err <= bound), f"max error / bound = {ratio}"


@pytest.mark.parametrize("case", ec.GEMM_SIGMOID_CASES, ids=lambda c: c.name)
def test_gemm_sigmoid_epilogue(lib, case):
    """RTK_SCORE_SIGMOID on rtk_gemm_f32 itself: float64 1 / (1 + exp(-z)) of the float64 product."""
    A, B = ec.gemm_operands(case)
    A, B = A * np.float32(2), B * np.float32(2)       # logits from ~0 to beyond +-10: the middle and both tails
    z = ec.gemm_ref(A, B)
    assert np.abs(z).max() > 4.0
    ref = 1.0 / (1.0 + np.exp(-z))
    got, _ = run_twice(lib, case, A, B, flags=1)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"\n[gemm sigmoid] {case.name}: max |dp| = {err:.3e}")
    assert err <= P_TOL
    logits, _ = run_twice(lib, case, A, B, flags=0)   # and the flag is what makes the difference
    assert np.all(np.abs(logits.astype(np.float64) - z) <= ec.gemm_bound(case, A, B))


def test_splitk_short_workspace_is_refused_and_c_untouched(lib):
    case = next(c for c in ec.GEMM_CASES if c.name == "splitk_s7")
    A, B = ec.gemm_operands(case)
    ta, pa, lda = lay_out(A, case.ak, case.a_pad, case.a_off)
    tb, pb, ldb = lay_out(B, case.bk, case.b_pad, case.b_off)
    ws = workspace(lib, case)
    need = lib.rtk_gemm_f32_splitk_workspace_bytes(case.M, case.N, case.splits)
    for given in (need - 1, 16, 0):
        buf, pc, ldc = new_c(case)
        assert call(lib, case, pa, lda, pb, ldb, pc, ldc, 0, ws, ws_bytes=given) == RTK_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert torch.all(buf == SENTINEL)
    buf, pc, ldc = new_c(case)
    assert call(lib, case, pa, lda, pb, ldb, pc, ldc, 0, None, ws_bytes=need) == RTK_ERR_WORKSPACE       # no workspace at all
    # a workspace off its 16-byte alignment is refused with the same status
    big = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.rtk_gemm_f32_splitk(pa, case.ak, lda, pb, case.bk, ldb, pc, ldc, case.M, case.N, case.K, case.splits,
                                 big.data_ptr() + 4, need, _stream())
    assert rc == RTK_ERR_WORKSPACE
    # ldc != N is not what the split-K form takes
    assert lib.rtk_gemm_f32_splitk(pa, case.ak, lda, pb, case.bk, ldb, pc, ldc + 1, case.M, case.N, case.K, case.splits,
                                   ws.data_ptr(), ws.numel(), _stream()) == -1
    torch.cuda.synchronize()
    assert torch.all(buf == SENTINEL)
    assert call(lib, case, pa, lda, pb, ldb, pc, ldc, 0, ws) == 0                                          # and the full one is taken
    torch.cuda.synchronize()
    assert np.array_equal(read_c(case, buf, ldc).astype(np.float64), ec.gemm_ref(A, B))
