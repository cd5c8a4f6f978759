"""The matrix-free BCE loss kernels on bf16 operands through their C entry points (rtk_bce_stream_rows_part_bf16,
rtk_bce_stream_grad_o_part_bf16, rtk_bce_stream_bf16_workspace_bytes) on bf16 planes packed from a given v
(rtk_pack_query_vectors): no stage 1 and no GEMM enters any bound.  The whole matrix is the block (0, N).

Cases, float64 references and the derived per-element bounds: tests/golden/bce_stream_bf16_cases.py (proved on the host
by tests/test_bce_stream_bf16_cases_host.py, mutants included).  Every case runs under both logistics; rows, dv and gO
are held to their bounds per element and the largest error / bound is printed.  Guards behind every output are NaN
before and afterwards, gO is -7.0 before and has to be written in full, the error word stays 0, a second run gives the
same bits.
"""
import functools

import numpy as np
import pytest
import torch

import bce_stream_bf16_cases as bb
import ce_kernel_cases as cc

pytestmark = pytest.mark.gpu

GUARD = 64
by_name = dict(ids=lambda c: c.name)
BAD_ARG, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def flags_of(mode):
    from r_tucker_amd import _lib
    return _lib.RTK_SCORE_SIGMOID | (_lib.RTK_SCORE_SIGMOID_FAST if mode == "fast" else 0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def dev_bf16(a):
    """bf16-exact float32 values as a bfloat16 tensor with those bits."""
    return dev(bb.bf16_bits(a).view(np.int16)).view(torch.bfloat16)


def nan_buf(n, dtype):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def setup(case):
    """Operands and the float64 references with their bounds (both logistics), computed once per case and shared."""
    data = bb.operands(case)
    bb.assert_unambiguous(case, data)
    return data, {mode: bb.bounds(case, data, mode == "fast") for mode in bb.MODES}


class Device:
    """The operands of a case on the device: bf16 planes packed from the fp32 v, O in bf16, the fp32 v, the CSR (global
    ids), the scalar scale."""

    def __init__(self, lib, case, data, mode):
        from r_tucker_amd import _lib
        self.case, self.lib, self.flags = case, lib, flags_of(mode)
        B, c = case.B, case.c
        self.v, self.O = dev(data.v), dev_bf16(data.O)
        self.qp = torch.empty(lib.rtk_packed_query_bytes(_lib.RTK_BF16, B, c), dtype=torch.uint8, device="cuda")
        assert lib.rtk_pack_query_vectors(self.v.data_ptr(), B, c, _lib.RTK_BF16, self.qp.data_ptr(), _stream()) == 0, \
            lib.rtk_last_error_string()
        self.keep = dev(data.csr.slot), dev(data.csr.ptr), dev(data.csr.obj)
        self.csr_p = [t.data_ptr() for t in self.keep]
        self.scale = dev(np.array([bb.scale_of(case)], dtype=np.float32))

    def workspace(self, n_local, max_pos):
        n = self.lib.rtk_bce_stream_bf16_workspace_bytes(self.case.B, n_local, self.case.c, max_pos)
        assert n > 0
        ws = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")           # 256 guard bytes behind it
        ws[:n] = 0
        return ws, n

    def o_rows(self, col0):
        ptr = self.O.data_ptr() + 2 * col0 * self.case.c
        assert ptr % 16 == 0                                    # c % 8 == 0: every row starts on 16 bytes
        return ptr

    def rows(self, block=None, want_dv=True):
        """-> (loss_rows with its guard, dv with its guard); block = (col0, n_local), None: the whole range."""
        case = self.case
        col0, n_local = block or (0, case.N)
        ws, n = self.workspace(n_local, 0)
        rows, dv = nan_buf(case.B, torch.float64), nan_buf(case.B * case.c, torch.float32)
        rc = self.lib.rtk_bce_stream_rows_part_bf16(self.qp.data_ptr(), case.B, case.c, self.o_rows(col0), n_local, col0,
                                                    case.N, *self.csr_p, case.eps, self.flags, rows.data_ptr(),
                                                    dv.data_ptr() if want_dv else None, ws.data_ptr(), n, _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0 and bool((ws[n:] == 0xA5).all()), "error word / workspace guard"
        return rows.cpu().numpy(), dv.cpu().numpy()

    def grad_o(self, max_pos, block=None):
        """-> (gO with its guard, error word); gO is -7.0 before."""
        case = self.case
        col0, n_local = block or (0, case.N)
        ws, n = self.workspace(n_local, max_pos)
        gO = nan_buf(n_local * case.c, torch.float32)
        gO[:n_local * case.c] = -7.0
        rc = self.lib.rtk_bce_stream_grad_o_part_bf16(self.qp.data_ptr(), self.v.data_ptr(), case.B, case.c,
                                                      self.o_rows(col0), n_local, col0, case.N, *self.csr_p, max_pos,
                                                      case.eps, self.flags, self.scale.data_ptr(), gO.data_ptr(),
                                                      ws.data_ptr(), n, _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        assert bool((ws[n:] == 0xA5).all()), "written behind the workspace"
        return gO.cpu().numpy(), int(ws[:4].view(torch.int32).item())

    def probabilities(self):
        """The stored fp32 probabilities of rtk_score_packed_bf16 on the same planes and O."""
        case = self.case
        P = torch.empty((case.B, case.N), dtype=torch.float32, device="cuda")
        rc = self.lib.rtk_score_packed_bf16(self.qp.data_ptr(), case.B, case.c, self.O.data_ptr(), case.N, P.data_ptr(),
                                            case.N, self.flags, _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        return P.cpu().numpy()


def run_block(d, data, block=None):
    """All the calls on one block with the checks every result has to pass -> (rows (B,), dv (B, c), gO (n_local, c))."""
    case = d.case
    B, c = case.B, case.c
    n_local = block[1] if block else case.N
    rows, dv = d.rows(block)
    rows2, dv2 = d.rows(block)
    assert np.array_equal(bits64(rows), bits64(rows2)) and np.array_equal(bits(dv), bits(dv2)), \
        "second rows run differs in its bits"
    assert np.isnan(rows[B:]).all() and np.isnan(dv[B * c:]).all(), "written past an output"
    rows3, dv3 = d.rows(block, want_dv=False)
    assert np.array_equal(bits64(rows3), bits64(rows)), "dv_out = NULL changes the bits of loss_rows"
    assert np.isnan(dv3).all(), "dv_out = NULL, and a dv buffer was written"
    longest, entries = data.csr.longest(), int(data.csr.stored().sum())
    gO, err = d.grad_o(B * longest, block)
    assert err == 0
    assert np.isnan(gO[n_local * c:]).all(), "written past gO"
    assert not (gO[:n_local * c] == -7.0).any(), "gO is not written in full"
    gO2, err2 = d.grad_o(B * longest, block)
    assert err2 == 0 and np.array_equal(bits(gO), bits(gO2)), "second grad_o run differs in its bits"
    gO3, err3 = d.grad_o(entries, block)
    assert err3 == 0 and np.array_equal(bits(gO), bits(gO3)), "max_pos = the batch's CSR entries differs from B * longest"
    return rows[:B], dv[:B * c].reshape(B, c), gO[:n_local * c].reshape(n_local, c)


@pytest.mark.parametrize("mode", bb.MODES)
@pytest.mark.parametrize("case", bb.CASES, **by_name)
def test_whole_range_against_float64(lib, case, mode):
    """rows, dv and gO per element; family S: the all-saturated rows have a dv row of zero bits and the columns that
    saturate for every query a gO row of +0.0 (bce_stream_cases.verdict)."""
    data, refs = setup(case)
    rows, dv, gO = run_block(Device(lib, case, data, mode), data)
    r_rows, r_dv, r_gO = bb.verdict(refs[mode], rows, dv, gO)
    print(f"\n[bce stream bf16] {case.name} {mode}: max error / bound = {r_rows:.4f} (loss_rows), {r_dv:.4f} (dv), "
          f"{r_gO:.4f} (gO)")
    assert r_rows <= 1.0 and r_dv <= 1.0 and r_gO <= 1.0


@pytest.mark.parametrize("mode", bb.MODES)
@pytest.mark.parametrize("case", bb.KS_CASES + [bb.SIGMA6_CASE, bb.SHAPE_CASES[3], bb.SHAPE_CASES[7], bb.S_CASES[1]], **by_name)
def test_loss_rows_against_the_stored_probabilities(lib, case, mode):
    """The loss rows against the float64 BCE of the device's own rtk_score_packed_bf16 probabilities, at the rows bound
    with dz = dp = 0: the chain order and the logistic are the score kernel's."""
    data, _ = setup(case)
    d = Device(lib, case, data, mode)
    ref, bound = bb.rows_from_probabilities(case, data, d.probabilities())
    rows, _ = d.rows(want_dv=False)
    r = cc._ratio(np.abs(rows[:case.B] - ref), bound)
    print(f"\n[bce stream bf16] {case.name} {mode}: loss_rows against the stored probabilities, error / bound = {r:.4f}")
    assert r <= 1.0


def run_partition(lib, part, mode):
    case = part.case
    data, refs = setup(case)
    d = Device(lib, case, data, mode)
    rows_sum, dv_sum, gO_rows = np.zeros(case.B), np.zeros((case.B, case.c), dtype=np.float32), []
    for block in part.blocks:
        rows, dv, gO = run_block(d, data, block)
        rows_sum = rows_sum + rows                              # float64 / fp32, block order: what an all-reduce SUM does
        dv_sum = dv_sum + dv
        gO_rows.append(gO)
    return bb.verdict(refs[mode], rows_sum, dv_sum, np.concatenate(gO_rows, axis=0))


@pytest.mark.parametrize("mode", bb.MODES)
@pytest.mark.parametrize("part", bb.PART_CASES, **by_name)
def test_blocks_against_float64(lib, part, mode):
    """Shares summed (rows, dv) and concatenated (gO) against the whole-range reference at twice its bound."""
    r_rows, r_dv, r_gO = run_partition(lib, part, mode)
    print(f"\n[bce stream bf16 part] {part.name} {mode}: max error / bound = {r_rows:.4f} (loss_rows), {r_dv:.4f} (dv), "
          f"{r_gO:.4f} (gO), allowance 2")
    assert r_rows <= 2.0 and r_dv <= 2.0 and r_gO <= 2.0


@pytest.mark.parametrize("mode", bb.MODES)
def test_small_blocks_and_the_wrong_smoothing_term(lib, mode):
    """n_ent = 64 in two blocks of 32, eps = 0.5: inside the doubled bound, which t0 = eps / n_local would leave by the
    printed factor (computed on the host)."""
    r = run_partition(lib, bb.MUTANT_PART, mode)
    factor = bb.smoothing_miss_factor()
    print(f"\n[bce stream bf16 part] {bb.MUTANT_PART.name} {mode}: max error / bound = {r[0]:.4f} (loss_rows), {r[1]:.4f} (dv), "
          f"{r[2]:.4f} (gO), allowance 2; t0 = eps / n_local would miss it by a factor of {factor:.4g}")
    assert max(r) <= 2.0 and factor >= 10.0


def test_more_entries_than_max_pos_set_bit_3(lib):
    """max_pos one below the batch's CSR entries: bit 3 (value 8) of the error word, nothing written past gO or behind
    the workspace (Device.grad_o checks its guard bytes)."""
    case = bb.SIGMA6_CASE
    data, _ = setup(case)
    d = Device(lib, case, data, "fast")
    entries = int(data.csr.stored().sum())
    for block, n_local in ((None, case.N), ((45, 50), 50)):
        gO, err = d.grad_o(entries - 1, block)
        assert err == 8
        assert np.isnan(gO[n_local * case.c:]).all(), "written past gO"
        assert d.grad_o(entries, block)[1] == 0


def test_workspace_bytes_answer_for_the_covered_shapes_only(lib):
    f = lib.rtk_bce_stream_bf16_workspace_bytes
    assert f(33, 97, 512, 100) > 0 and f(0, 1, 8, 0) > 0
    for bad in ((33, 97, 520, 100), (33, 97, 20, 100), (33, 97, 0, 100), (-1, 97, 16, 0), (33, 0, 16, 0), (33, 97, 16, -1)):
        assert f(*bad) == 0, bad
    assert f(33, 97, 512, 100) % 256 == 0 and f(33, 97, 512, 1000) > f(33, 97, 512, 100)
    # the fp32 forms keep their answers
    assert lib.rtk_bce_stream_part_workspace_bytes(33, 97, 512, 100) == 0
    assert lib.rtk_bce_stream_part_workspace_bytes(33, 97, 208, 100) == lib.rtk_bce_stream_workspace_bytes(33, 97, 208, 100) > 0


def test_refusals_leave_the_outputs_untouched(lib):
    case = bb.UNIT_SCALE_CASE                                   # B 33, N 97, c 16
    data, _ = setup(case)
    d = Device(lib, case, data, "fast")
    B, N, c, fl = case.B, case.N, case.c, flags_of("fast")
    max_pos = B * data.csr.longest()
    need = max(lib.rtk_bce_stream_bf16_workspace_bytes(B, N, c, max_pos), lib.rtk_bce_stream_bf16_workspace_bytes(B, N, 512, max_pos))
    exact = lib.rtk_bce_stream_bf16_workspace_bytes(B, N, c, max_pos)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rows = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    dv = torch.full((B, c), -7.0, device="cuda")
    gO = torch.full((N, c), -7.0, device="cuda")
    Obuf = torch.zeros(N * c + 16, dtype=torch.bfloat16, device="cuda")
    Obuf[1:N * c + 1] = d.O.reshape(-1)
    base = dict(c=c, O=d.O.data_ptr(), n_local=N, col0=0, eps=0.1, flags=fl, nbytes=need, batch=B)

    def call(which, **kw):
        a = dict(base, **kw)
        block = (a["n_local"], a["col0"], N)
        if which == "rows":
            return lib.rtk_bce_stream_rows_part_bf16(d.qp.data_ptr(), a["batch"], a["c"], a["O"], *block, *d.csr_p, a["eps"],
                                                     a["flags"], rows.data_ptr(), dv.data_ptr(), ws.data_ptr(), a["nbytes"],
                                                     _stream())
        return lib.rtk_bce_stream_grad_o_part_bf16(d.qp.data_ptr(), d.v.data_ptr(), a["batch"], a["c"], a["O"], *block,
                                                   *d.csr_p, max_pos, a["eps"], a["flags"], d.scale.data_ptr(), gO.data_ptr(),
                                                   ws.data_ptr(), a["nbytes"], _stream())

    for which in ("rows", "grad_o"):
        assert call(which, c=520) == UNSUPPORTED and b"512" in lib.rtk_last_error_string()
        assert call(which, c=20) == UNSUPPORTED and b"c % 8" in lib.rtk_last_error_string()
        assert call(which, O=Obuf.data_ptr() + 2) == UNSUPPORTED and b"aligned" in lib.rtk_last_error_string()
        assert call(which, eps=1.0) == BAD_ARG and b"label smoothing" in lib.rtk_last_error_string()
        assert call(which, flags=fl & ~1) == UNSUPPORTED and b"RTK_SCORE_SIGMOID" in lib.rtk_last_error_string()
        short = (exact if which == "grad_o" else lib.rtk_bce_stream_bf16_workspace_bytes(B, N, c, 0)) - 256
        assert call(which, nbytes=short) == BAD_ARG and b"workspace" in lib.rtk_last_error_string()
        assert call(which, col0=1) == BAD_ARG and b"block" in lib.rtk_last_error_string()
        assert call(which, col0=N - 16, n_local=17) == BAD_ARG and b"block" in lib.rtk_last_error_string()
        assert call(which, batch=-1) == BAD_ARG and b"batch" in lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((dv == -7.0).all()) and bool((gO == -7.0).all())
    assert not ws.any(), "a refused call touched the workspace"
    # batch == 0: rows returns at once, grad_o zeroes gO
    assert call("rows", batch=0) == 0 and call("grad_o", batch=0) == 0
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((dv == -7.0).all()) and not gO.any() and not ws.any()
    gO.fill_(-7.0)
    assert call("rows") == 0 and call("grad_o") == 0            # the same arguments without a fault are accepted
    torch.cuda.synchronize()
    assert not bool((rows == -7.0).any()) and not bool((gO == -7.0).any())
