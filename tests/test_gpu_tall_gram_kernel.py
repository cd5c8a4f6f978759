"""rtk_tall_gram_f64 (csrc/rtk_tall_gram.hip) through its C ABI on every case of tests/golden/tall_gram_cases.py:
family E bit-equal to the float64 reference, family G inside ``2 * 1.01 * n * u * |A|^T |B|`` per entry.
tests/test_tall_gram_cases_host.py proves on the host that these bounds hold for any summation order and that every
defect the kernel could have leaves them.

Every launch: the operand buffers hold NaN everywhere outside the (n x p) and (n x q) windows (the rest of each row's
pitch, and 8 rows behind row n), C is pre-filled with NaN and followed by a sentinel, the workspace is followed by a
sentinel; so a read outside the windows or a write outside C shows in every case."""
import numpy as np
import pytest
import torch

import tall_gram_cases as tg

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.0e30
BAD_ARG, UNSUPPORTED = -1, -3
WORST = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def device_operand(buf, windows, ld_max):
    """``buf`` on the device with NaN everywhere outside ``windows`` ((off, ld, n, cols), ...) and 8 rows of NaN behind."""
    host = np.full(buf.size + 8 * ld_max, np.nan, dtype=np.float32)
    for off, ld, n, cols in windows:
        idx = off + np.arange(n, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]
        host[idx] = buf[idx]
    return torch.from_numpy(host).cuda()


def call(lib, pa, lda, pb, ldb, n, p, q, expect=0, c_ptr=None, ws_ptr=None, ws_bytes=None, pq_alloc=None):
    """One call on device pointers -> C as the call left it; C pre-filled with NaN, sentinels behind C and the
    workspace.  ``expect`` != 0: the call must return that status and leave C and the workspace as they were."""
    pp, qq = pq_alloc or (p, q)
    need = max(tg.workspace_bytes(n, p, q), tg.workspace_bytes(max(n, 0), pp, qq), 256)
    assert lib.rtk_tall_gram_f64_workspace_bytes(n, p, q) == tg.workspace_bytes(n, p, q)
    C = torch.full((pp * qq + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    C[pp * qq:] = SENTINEL
    ws = torch.full((need // 8 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    c0, w0 = C.cpu().numpy(), ws.cpu().numpy()
    rc = lib.rtk_tall_gram_f64(pa, lda, pb, ldb, n, p, q, C.data_ptr() if c_ptr is None else c_ptr(C.data_ptr()),
                               ws.data_ptr() if ws_ptr is None else ws_ptr(ws.data_ptr()),
                               need if ws_bytes is None else ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, lib.rtk_last_error_string())
    torch.cuda.synchronize()
    c1, w1 = C.cpu().numpy(), ws.cpu().numpy()
    assert np.array_equal(bits(c1[pp * qq:]), bits(c0[pp * qq:])), "written past C"
    assert np.array_equal(bits(w1[need // 8:]), bits(w0[need // 8:])), "written past the workspace"
    if expect:
        assert np.array_equal(bits(c1), bits(c0)) and np.array_equal(bits(w1), bits(w0)), "a refused call wrote"
    return c1[:pp * qq].reshape(pp, qq)


def run_case(lib, case, n=None, row0=0):
    """The kernel on a case (or on its rows [row0, row0 + n)) -> C."""
    op = tg.operands(case)
    n = case.n if n is None else n
    wa, wb = (op.off_a, op.lda, case.n, case.p), (op.off_b, op.ldb, case.n, case.q)
    if op.buf_a is op.buf_b:
        da = db = device_operand(op.buf_a, (wa, wb), max(op.lda, op.ldb))
    else:
        da, db = device_operand(op.buf_a, (wa,), op.lda), device_operand(op.buf_b, (wb,), op.ldb)
    pa = da.data_ptr() + 4 * (op.off_a + row0 * op.lda)
    pb = db.data_ptr() + 4 * (op.off_b + row0 * op.ldb)
    assert (pa % 16 == 0 and pb % 16 == 0) == (op.off_a % 4 == 0 and op.off_b % 4 == 0) or row0   # tg.vector_path's premise
    return call(lib, pa, op.lda, pb, op.ldb, n, case.p, case.q)


@pytest.mark.parametrize("case", tg.CASES, ids=lambda c: c.name)
def test_case_meets_its_bound(lib, case):
    C = run_case(lib, case)
    ok, worst = tg.inside(case, C)
    key = (case.family, "vec" if tg.vector_path(case) else "scalar")
    if worst > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (worst, case.name)
    print(f"{case.name}: " + (f"{int(worst)} entries differ" if case.family == "E" else f"error / bound = {worst:.4f}"))
    assert ok, (case.name, worst)


def test_report_worst_ratios():
    for key, (w, name) in sorted(WORST.items()):
        print(f"family {key[0]} {key[1]} path: worst {'differing entries' if key[0] == 'E' else 'error / bound'} {w:.4f} ({name})")


@pytest.mark.parametrize("name", ["G-n4099-200x200-contig", "G-n2500-512x512-halves", "G-n4099-20x12-odd"])
def test_two_calls_give_the_same_bits(lib, name):
    case = tg.BY_NAME[name]
    assert np.array_equal(bits(run_case(lib, case)), bits(run_case(lib, case)))


def test_row_blocks_add_up(lib):
    """Row blocks cut INSIDE the kernel's ranges (1024 rows here), each through the kernel, added in float64: within the
    sum of the blocks' bounds of the kernel's result on the whole."""
    case = tg.BY_NAME["G-n4099-200x200-contig"]
    A, B = tg.matrices(case)
    whole = run_case(lib, case)
    cuts = (0, 500, 1700, 4099)
    total, bnd = np.zeros_like(whole), np.zeros_like(whole)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        total = total + run_case(lib, case, n=hi - lo, row0=lo)
        bnd += 2 * 1.01 * (hi - lo) * tg.U * (np.abs(A[lo:hi]).astype(np.float64).T @ np.abs(B[lo:hi]).astype(np.float64))
    err = np.abs(total - whole)
    print(f"row blocks vs whole: worst error / bound = {(err / bnd).max():.4f}")
    assert (err <= bnd).all()


def test_non_finite_values_inside_propagate(lib):
    case = tg.BY_NAME["G-n2500-8x8-contig"]
    op = tg.operands(case)
    for value, row, col in ((np.nan, 0, 3), (np.inf, 2499, 7), (np.nan, 1500, 0)):
        a = op.buf_a.copy()
        a[row * op.lda + col] = value
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(op.buf_b).cuda()
        C = call(lib, da.data_ptr(), op.lda, db.data_ptr(), op.ldb, case.n, case.p, case.q)
        hit = ~np.isfinite(C)
        assert hit[col].all() and not np.delete(hit, col, axis=0).any(), (value, row, col)
        if np.isnan(value):
            assert np.isnan(C[col]).all()


def test_n_zero_writes_zeros(lib):
    d = torch.full((1024,), float("nan"), dtype=torch.float32, device="cuda")
    for p, q in ((1, 1), (20, 12), (200, 64)):
        C = call(lib, d.data_ptr(), p, d.data_ptr(), q, 0, p, q)
        assert np.array_equal(bits(C), bits(np.zeros((p, q))))


def test_refusals_leave_the_outputs_alone(lib):
    d = torch.ones(64 * 40, dtype=torch.float32, device="cuda")
    a = d.data_ptr()
    n, p, q = 64, 20, 12
    ok = dict(pa=a, lda=p, pb=a, ldb=q, n=n, p=p, q=q)
    for change, status in (
            (dict(pa=None), BAD_ARG), (dict(pb=None), BAD_ARG), (dict(c_ptr=lambda x: None), BAD_ARG),
            (dict(ws_ptr=lambda x: None), BAD_ARG), (dict(n=-1), BAD_ARG), (dict(lda=p - 1), BAD_ARG),
            (dict(ldb=q - 1), BAD_ARG), (dict(ws_bytes=tg.workspace_bytes(n, p, q) - 1), BAD_ARG),
            (dict(ws_bytes=0), BAD_ARG), (dict(ws_ptr=lambda x: x + 8), BAD_ARG),
            (dict(p=0, lda=1), UNSUPPORTED), (dict(q=0), UNSUPPORTED), (dict(p=1025, lda=1025), UNSUPPORTED),
            (dict(q=1025, ldb=1025), UNSUPPORTED)):
        kw = dict(ok, **change)
        call(lib, expect=status, pq_alloc=(p, q), **kw)
        assert lib.rtk_last_error_string().startswith(b"rtk_tall_gram_f64"), change
    assert lib.rtk_tall_gram_f64_workspace_bytes(n, 0, q) == 0 and lib.rtk_tall_gram_f64_workspace_bytes(n, p, 1025) == 0
    C = call(lib, **ok)                                   # and the same arguments, unchanged, are served
    assert np.array_equal(C, np.full((p, q), 64.0))


def test_peak_memory_is_the_workspace(lib):
    """No float64 copy of the operand: on a (65536 x 128) block the wrapper's peak is the workspace and C (the copy
    alone would be 64 MiB)."""
    from r_tucker_amd import smalllinalg as sl
    n, k = 65536, 128
    A = torch.randn((n, k), dtype=torch.float32, device="cuda")
    sl.tall_gram_f64_rows(A[:64], A[:64])                 # library and allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    C = sl.tall_gram_f64_rows(A, A)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    ws = tg.workspace_bytes(n, k, k)
    print(f"peak growth {growth} bytes; workspace {ws}, C {k * k * 8}; a float64 copy would be {n * k * 8}")
    assert growth <= ws + k * k * 8 + (1 << 20)
    assert ws + k * k * 8 + (1 << 20) < n * k * 8
    ref = A.double().T @ A.double()
    assert float((C - ref).abs().max()) <= 2 * 1.01 * n * tg.U * float((A.double().abs().T @ A.double().abs()).max())


def test_wrapper_takes_strided_views(lib):
    """``smalllinalg.tall_gram_f64_rows`` on the column halves of one matrix and on a view at an odd column: the pitch
    comes from the stride, nothing is copied, and the bits are those of the call on contiguous copies."""
    from r_tucker_amd import smalllinalg as sl
    f = torch.randn((3001, 40), dtype=torch.float32, device="cuda")
    for A, B in ((f[:, :20], f[:, 20:]), (f[:, 1:14], f[:, 3:40]), (f[:1, :8], f[:1, 8:24])):
        got = sl.tall_gram_f64_rows(A, B)
        want = sl.tall_gram_f64_rows(A.contiguous(), B.contiguous())
        assert got.shape == (A.shape[1], B.shape[1]) and torch.equal(got, want)
        assert torch.allclose(got, A.double().T @ B.double(), rtol=1e-12, atol=1e-12)
