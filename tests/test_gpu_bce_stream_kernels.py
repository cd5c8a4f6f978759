"""The matrix-free BCE loss kernels through their four C entry points (rtk_bce_stream_rows_f32,
rtk_bce_stream_grad_o_f32, rtk_bce_stream_rows_part_f32, rtk_bce_stream_grad_o_part_f32) on planes packed from a given
v (rtk_pack_query_vectors): no stage 1 and no GEMM enters any bound.

Cases, float64 references and the derived per-element bounds: tests/golden/bce_stream_cases.py (proved on the host by
tests/test_bce_stream_cases_host.py, mutants included).  Every case runs under both logistics; rows, dv and gO are held
to their bounds per element and the largest error / bound is printed.  Guards behind every output are NaN before and
afterwards, gO is -7.0 before and has to be written in full, the error word stays 0, a second run gives the same bits.
"""
import functools

import numpy as np
import pytest
import torch

import bce_stream_cases as bs

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


def nan_buf(n, dtype):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def setup(case):
    """Operands and the float64 references with their bounds (both logistics), computed once per case and shared."""
    data = bs.operands(case)
    bs.assert_unambiguous(case, data)
    return data, {mode: bs.bounds(case, data, mode == "fast") for mode in bs.MODES}


class Device:
    """The operands of a case on the device: packed planes, O, v, the CSR (global ids), the scalar scale."""

    def __init__(self, lib, case, data, mode):
        self.case, self.lib, self.flags = case, lib, flags_of(mode)
        B, c = case.B, case.c
        self.v, self.O = dev(data.v), dev(data.O)
        self.qp = torch.empty(lib.rtk_packed_query_bytes(0, B, c), dtype=torch.uint8, device="cuda")
        assert lib.rtk_pack_query_vectors(self.v.data_ptr(), B, c, 0, self.qp.data_ptr(), _stream()) == 0, \
            lib.rtk_last_error_string()
        self.keep = dev(data.csr.slot), dev(data.csr.ptr), dev(data.csr.obj)
        self.csr_p = [t.data_ptr() for t in self.keep]
        self.scale = dev(np.array([bs.scale_of(case)], dtype=np.float32))

    def workspace(self, n_local, max_pos, part):
        f = self.lib.rtk_bce_stream_part_workspace_bytes if part else self.lib.rtk_bce_stream_workspace_bytes
        n = f(self.case.B, n_local, self.case.c, max_pos)
        assert n > 0
        ws = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")           # 256 guard bytes behind it
        ws[:n] = 0
        return ws, n

    def o_rows(self, col0):
        ptr = self.O.data_ptr() + 4 * col0 * self.case.c
        assert ptr % 16 == 0                                    # c % 4 == 0: every row starts on 16 bytes
        return ptr

    def rows(self, block=None, want_dv=True):
        """-> (loss_rows with its guard, dv with its guard); block = (col0, n_local): the _part entry point."""
        case = self.case
        col0, n_local = block or (0, case.N)
        ws, n = self.workspace(n_local, 0, block is not None)
        rows, dv = nan_buf(case.B, torch.float64), nan_buf(case.B * case.c, torch.float32)
        tail = (case.eps, self.flags, rows.data_ptr(), dv.data_ptr() if want_dv else None, ws.data_ptr(), n, _stream())
        if block is None:
            rc = self.lib.rtk_bce_stream_rows_f32(self.qp.data_ptr(), case.B, case.c, self.O.data_ptr(), case.N, *self.csr_p,
                                                  *tail)
        else:
            rc = self.lib.rtk_bce_stream_rows_part_f32(self.qp.data_ptr(), case.B, case.c, self.o_rows(col0), n_local, col0,
                                                       case.N, *self.csr_p, *tail)
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0 and bool((ws[n:] == 0xA5).all()), "error word / workspace guard"
        return rows.cpu().numpy(), dv.cpu().numpy()

    def grad_o(self, max_pos, block=None):
        """-> (gO with its guard, error word); gO is -7.0 before."""
        case = self.case
        col0, n_local = block or (0, case.N)
        ws, n = self.workspace(n_local, max_pos, block is not None)
        gO = nan_buf(n_local * case.c, torch.float32)
        gO[:n_local * case.c] = -7.0
        tail = (max_pos, case.eps, self.flags, self.scale.data_ptr(), gO.data_ptr(), ws.data_ptr(), n, _stream())
        if block is None:
            rc = self.lib.rtk_bce_stream_grad_o_f32(self.qp.data_ptr(), self.v.data_ptr(), case.B, case.c, self.O.data_ptr(),
                                                    case.N, *self.csr_p, *tail)
        else:
            rc = self.lib.rtk_bce_stream_grad_o_part_f32(self.qp.data_ptr(), self.v.data_ptr(), case.B, case.c,
                                                         self.o_rows(col0), n_local, col0, case.N, *self.csr_p, *tail)
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        assert bool((ws[n:] == 0xA5).all()), "written behind the workspace"
        return gO.cpu().numpy(), int(ws[:4].view(torch.int32).item())


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


@pytest.mark.parametrize("mode", bs.MODES)
@pytest.mark.parametrize("case", bs.CASES, **by_name)
def test_whole_matrix_against_float64(lib, case, mode):
    """rows, dv and gO per element; family S: the all-saturated rows have a dv row of zero bits and the columns that
    saturate for every query a gO row of +0.0 (bce_stream_cases.verdict)."""
    data, refs = setup(case)
    rows, dv, gO = run_block(Device(lib, case, data, mode), data)
    r_rows, r_dv, r_gO = bs.verdict(refs[mode], rows, dv, gO)
    print(f"\n[bce stream] {case.name} {mode}: max error / bound = {r_rows:.4f} (loss_rows), {r_dv:.4f} (dv), {r_gO:.4f} (gO)")
    assert r_rows <= 1.0 and r_dv <= 1.0 and r_gO <= 1.0


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
    return bs.verdict(refs[mode], rows_sum, dv_sum, np.concatenate(gO_rows, axis=0))


@pytest.mark.parametrize("mode", bs.MODES)
@pytest.mark.parametrize("part", bs.PART_CASES, **by_name)
def test_blocks_against_float64(lib, part, mode):
    """Shares summed (rows, dv) and concatenated (gO) against the whole-matrix reference at twice its bound."""
    r_rows, r_dv, r_gO = run_partition(lib, part, mode)
    print(f"\n[bce stream part] {part.name} {mode}: max error / bound = {r_rows:.4f} (loss_rows), {r_dv:.4f} (dv), "
          f"{r_gO:.4f} (gO), allowance 2")
    assert r_rows <= 2.0 and r_dv <= 2.0 and r_gO <= 2.0


@pytest.mark.parametrize("mode", bs.MODES)
def test_small_blocks_and_the_wrong_smoothing_term(lib, mode):
    """n_ent = 64 in two blocks of 32, eps = 0.5: inside the doubled bound, which t0 = eps / n_local would leave by the
    printed factor (computed on the host)."""
    r = run_partition(lib, bs.MUTANT_PART, mode)
    factor = bs.smoothing_miss_factor()
    print(f"\n[bce stream part] {bs.MUTANT_PART.name} {mode}: max error / bound = {r[0]:.4f} (loss_rows), {r[1]:.4f} (dv), "
          f"{r[2]:.4f} (gO), allowance 2; t0 = eps / n_local would miss it by a factor of {factor:.4g}")
    assert max(r) <= 2.0 and factor >= 10.0


@pytest.mark.parametrize("mode", bs.MODES)
@pytest.mark.parametrize("case", bs.WHOLE_BLOCK_CASES, **by_name)
def test_the_block_of_all_rows_has_the_whole_matrix_bits(lib, case, mode):
    data, _ = setup(case)
    d = Device(lib, case, data, mode)
    max_pos = case.B * data.csr.longest()
    rows, dv = d.rows()
    rows_p, dv_p = d.rows((0, case.N))
    assert np.array_equal(bits64(rows), bits64(rows_p)) and np.array_equal(bits(dv), bits(dv_p))
    (gO, err), (gO_p, err_p) = d.grad_o(max_pos), d.grad_o(max_pos, (0, case.N))
    assert err == 0 and err_p == 0 and np.array_equal(bits(gO), bits(gO_p))


@pytest.mark.parametrize("part", [False, True], ids=["whole", "part"])
def test_more_entries_than_max_pos_set_bit_3(lib, part):
    """max_pos one below the batch's CSR entries: bit 3 (value 8) of the error word, nothing written past gO or behind
    the workspace (Device.grad_o checks its guard bytes)."""
    case = bs.SIGMA6_CASE
    data, _ = setup(case)
    d = Device(lib, case, data, "fast")
    entries = int(data.csr.stored().sum())
    block = (45, 50) if part else None
    n_local = 50 if part else case.N
    gO, err = d.grad_o(entries - 1, block)
    assert err == 8
    assert np.isnan(gO[n_local * case.c:]).all(), "written past gO"
    assert d.grad_o(entries, block)[1] == 0


def test_refusals_leave_the_outputs_untouched(lib):
    case = bs.UNIT_SCALE_CASE                                   # B 31, N 33, c 16
    data, _ = setup(case)
    d = Device(lib, case, data, "fast")
    B, N, c, fl = case.B, case.N, case.c, flags_of("fast")
    max_pos = B * data.csr.longest()
    need = lib.rtk_bce_stream_workspace_bytes(B, N, c, max_pos)
    assert need == lib.rtk_bce_stream_part_workspace_bytes(B, N, c, max_pos)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rows = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    dv = torch.full((B, c), -7.0, device="cuda")
    gO = torch.full((N, c), -7.0, device="cuda")
    Obuf = torch.zeros(N * c + 4, device="cuda")
    Obuf[1:N * c + 1] = d.O.reshape(-1)
    base = dict(c=c, O=d.O.data_ptr(), n_local=N, col0=0, eps=0.1, flags=fl, nbytes=need)

    def call(which, part, **kw):
        a = dict(base, **kw)
        block = (a["n_local"], a["col0"], N) if part else (N,)
        if which == "rows":
            f = lib.rtk_bce_stream_rows_part_f32 if part else lib.rtk_bce_stream_rows_f32
            return f(d.qp.data_ptr(), B, a["c"], a["O"], *block, *d.csr_p, a["eps"], a["flags"], rows.data_ptr(), dv.data_ptr(),
                     ws.data_ptr(), a["nbytes"], _stream())
        f = lib.rtk_bce_stream_grad_o_part_f32 if part else lib.rtk_bce_stream_grad_o_f32
        return f(d.qp.data_ptr(), d.v.data_ptr(), B, a["c"], a["O"], *block, *d.csr_p, max_pos, a["eps"], a["flags"],
                 d.scale.data_ptr(), gO.data_ptr(), ws.data_ptr(), a["nbytes"], _stream())

    for which in ("rows", "grad_o"):
        for part in (False, True):
            assert call(which, part, c=212) == UNSUPPORTED and b"208" in lib.rtk_last_error_string()
            assert call(which, part, c=18) == UNSUPPORTED and b"c % 4" in lib.rtk_last_error_string()
            assert call(which, part, O=Obuf.data_ptr() + 4) == UNSUPPORTED and b"aligned" in lib.rtk_last_error_string()
            assert call(which, part, eps=1.0) == BAD_ARG and b"label smoothing" in lib.rtk_last_error_string()
            assert call(which, part, flags=fl & ~1) == UNSUPPORTED and b"RTK_SCORE_SIGMOID" in lib.rtk_last_error_string()
            short = (need if which == "grad_o" else lib.rtk_bce_stream_workspace_bytes(B, N, c, 0)) - 256
            assert call(which, part, nbytes=short) == BAD_ARG and b"workspace" in lib.rtk_last_error_string()
        assert call(which, True, col0=1) == BAD_ARG and b"block" in lib.rtk_last_error_string()
        assert call(which, True, col0=N - 16, n_local=17) == BAD_ARG and b"block" in lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert bool((rows == -7.0).all()) and bool((dv == -7.0).all()) and bool((gO == -7.0).all())
    assert not ws.any(), "a refused call touched the workspace"
    assert call("rows", True) == 0 and call("grad_o", True) == 0       # the same arguments without a fault are accepted
    torch.cuda.synchronize()
    assert not bool((rows == -7.0).any()) and not bool((gO == -7.0).any())
