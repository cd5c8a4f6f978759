"""The block form of the matrix-free cross-entropy kernels through its C entry points (rtk_ce_stream_rows_part_f32,
rtk_ce_stream_grad_part_f32) on planes packed from a given v: no stage 1 and no GEMM enters any bound.

  * one block that is the whole matrix: grad_part has the bits of rtk_ce_stream_grad_f32 (dv, gO, the error word), and
    the block's (m, s, lin) give that call's lse_out within one float32 ulp and its loss rows within
    2^-48 (|w lse| + |lin| + 1);
  * proper blocks against float64, per block (m, m + ln s, lin) and merged (lse), then the backward from the global lse:
    dv shares summed and gO concatenated, judged by ce_kernel_cases.stream_backward_verdict at twice its bound.

Cases, references and the derived bounds: tests/golden/ce_part_cases.py (tests/test_ce_part_cases_host.py shows on the
host that the named mutants leave them).  Guards behind every output are NaN before and afterwards; a second run gives
the same bits."""
import functools

import numpy as np
import pytest
import torch

import ce_kernel_cases as cc
import ce_part_cases as pc

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
    """The operands and the whole-matrix float64 forward, computed once per case and shared."""
    data = cc.stream_operands(case)
    fwd = cc.stream_forward(case, data)
    return data, fwd, fwd[0].astype(np.float32)


class Device:
    """The operands of a case on the device: packed planes, O, v, the CSR (global ids)."""

    def __init__(self, lib, case, data):
        self.case, self.lib = case, lib
        B, c = case.B, case.c
        self.v, self.O = dev(data.v), dev(data.O)
        self.qp = torch.empty(lib.rtk_packed_query_bytes(0, B, c), dtype=torch.uint8, device="cuda")
        assert lib.rtk_pack_query_vectors(self.v.data_ptr(), B, c, 0, self.qp.data_ptr(), _stream()) == 0, \
            lib.rtk_last_error_string()
        self.keep = dev(data.csr.slot), dev(data.csr.ptr), dev(data.csr.obj)
        self.csr_p = [t.data_ptr() for t in self.keep]
        self.scale = dev(np.array([cc.stream_scale(case)], dtype=np.float32))

    def _ws(self, n_local, max_pos):
        n = self.lib.rtk_ce_stream_part_workspace_bytes(self.case.B, n_local, self.case.c, max_pos)
        assert n > 0
        return torch.zeros(n, dtype=torch.uint8, device="cuda")

    def o_rows(self, col0):
        ptr = self.O.data_ptr() + 4 * col0 * self.case.c
        assert ptr % 16 == 0                                    # c % 4 == 0: every row starts on 16 bytes
        return ptr

    def rows_part(self, col0, n_local):
        """-> (m, s, lin) with their guards."""
        case, ws = self.case, self._ws(n_local, 0)
        m, s, lin = nan_buf(case.B, torch.float32), nan_buf(case.B, torch.float64), nan_buf(case.B, torch.float64)
        rc = self.lib.rtk_ce_stream_rows_part_f32(self.qp.data_ptr(), case.B, case.c, self.o_rows(col0), n_local, col0, case.N,
                                                  *self.csr_p, case.eps, m.data_ptr(), s.data_ptr(), lin.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        return m.cpu().numpy(), s.cpu().numpy(), lin.cpu().numpy()

    def grad_part(self, col0, n_local, lse32, max_pos):
        """-> (dv with its guard, the block's gO with its guard, error word); gO is -7.0 before."""
        case, ws = self.case, self._ws(n_local, max_pos)
        lse_d = dev(lse32)
        dv = nan_buf(case.B * case.c, torch.float32)
        gO = nan_buf(n_local * case.c, torch.float32)
        gO[:n_local * case.c] = -7.0
        rc = self.lib.rtk_ce_stream_grad_part_f32(self.qp.data_ptr(), self.v.data_ptr(), case.B, case.c, self.o_rows(col0),
                                                  n_local, col0, case.N, *self.csr_p, max_pos, case.eps, lse_d.data_ptr(),
                                                  self.scale.data_ptr(), dv.data_ptr(), gO.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), _stream())
        assert rc == 0, self.lib.rtk_last_error_string()
        torch.cuda.synchronize()
        return dv.cpu().numpy(), gO.cpu().numpy(), int(ws[:4].view(torch.int32).item())

    def whole(self, max_pos):
        """rtk_ce_stream_rows_f32, then rtk_ce_stream_grad_f32 from its lse_out -> (rows, lse, dv, gO, error word)."""
        case, lib = self.case, self.lib
        n = lib.rtk_ce_stream_workspace_bytes(case.B, case.N, case.c, max_pos)
        ws = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rows, lse = nan_buf(case.B, torch.float64), nan_buf(case.B, torch.float32)
        rc = lib.rtk_ce_stream_rows_f32(self.qp.data_ptr(), case.B, case.c, self.O.data_ptr(), case.N, *self.csr_p, case.eps,
                                        rows.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, lib.rtk_last_error_string()
        dv = nan_buf(case.B * case.c, torch.float32)
        gO = nan_buf(case.N * case.c, torch.float32)
        rc = lib.rtk_ce_stream_grad_f32(self.qp.data_ptr(), self.v.data_ptr(), case.B, case.c, self.O.data_ptr(), case.N,
                                        *self.csr_p, max_pos, case.eps, lse.data_ptr(), self.scale.data_ptr(), dv.data_ptr(),
                                        gO.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        assert rc == 0, lib.rtk_last_error_string()
        torch.cuda.synchronize()
        return rows.cpu().numpy(), lse.cpu().numpy(), dv.cpu().numpy(), gO.cpu().numpy(), int(ws[:4].view(torch.int32).item())


WHOLE_CASES = [cc.StreamCase("G", 70, 3003, 200), cc.StreamCase("G", 33, 3003, 208)]


@pytest.mark.parametrize("case", WHOLE_CASES, **by_name)
def test_one_block_is_the_whole_call(lib, case):
    data, _, _ = setup(case)
    d = Device(lib, case, data)
    B, N, c = case.B, case.N, case.c
    max_pos = B * data.csr.longest()
    rows, lse, dv, gO, err = d.whole(max_pos)
    assert err == 0
    dvp, gOp, errp = d.grad_part(0, N, lse[:B].copy(), max_pos)
    assert errp == err and np.array_equal(bits(dvp), bits(dv)) and np.array_equal(bits(gOp), bits(gO)), \
        "grad_part on the block (0, n_ent) differs from rtk_ce_stream_grad_f32 in its bits"
    m, s, lin = d.rows_part(0, N)
    assert np.isnan(m[B:]).all() and np.isnan(s[B:]).all() and np.isnan(lin[B:]).all(), "written past row B"
    m, s, lin = m[:B], s[:B], lin[:B]
    lse_b = m.astype(np.float64) + np.log(s)
    ulp = np.spacing(np.abs(lse[:B])).astype(np.float64)
    d_lse = np.abs(lse_b - lse[:B].astype(np.float64))
    _, dt, eps = cc.consts64(N, case.eps)
    w = cc.weights(data.csr.stored(), dt, eps)
    d_rows = np.abs(w * lse_b + lin - rows[:B])
    allow = 2.0 ** -48 * (np.abs(w * lse_b) + np.abs(lin) + 1.0)
    print(f"\n[ce part = whole] {case.name}: lse off by {float((d_lse / ulp).max()):.3f} ulp, rows by "
          f"{float((d_rows / allow).max()):.4f} of 2^-48 (|w lse| + |lin| + 1)")
    assert np.all(d_lse <= ulp) and np.all(d_rows <= allow)


@pytest.mark.parametrize("part", pc.PART_CASES, **by_name)
def test_blocks_against_float64(lib, part):
    case = part.case
    data, fwd, lse32 = setup(case)
    d = Device(lib, case, data)
    B, N, c = case.B, case.N, case.c
    max_pos = B * data.csr.longest()
    ms, ss, worst = [], [], [0.0, 0.0]
    dv_sum = np.zeros((B, c), dtype=np.float32)
    gO_rows = []
    for col0, n_local in part.blocks:
        m, s, lin = d.rows_part(col0, n_local)
        m2, s2, lin2 = d.rows_part(col0, n_local)
        assert np.array_equal(bits(m), bits(m2)) and np.array_equal(bits64(s), bits64(s2)) and \
            np.array_equal(bits64(lin), bits64(lin2)), "second forward run differs in its bits"
        assert np.isnan(m[B:]).all() and np.isnan(s[B:]).all() and np.isnan(lin[B:]).all(), "written past row B"
        ref = pc.block_forward(case, data, col0, n_local)
        m_ok, r_lse, r_lin = pc.block_forward_verdict(case, ref, m[:B], s[:B], lin[:B])
        print(f"\n[ce part rows] {part.name} block ({col0}, {n_local}): m {'ok' if m_ok else 'OUT'}, max error / bound = "
              f"{r_lse:.4f} (m + ln s), {r_lin:.4f} (lin)")
        assert m_ok and r_lse <= 1.0 and r_lin <= 1.0
        worst = [max(worst[0], r_lse), max(worst[1], r_lin)]
        ms.append(m[:B])
        ss.append(s[:B])
        # the backward of the block, from the GLOBAL lse
        dv, gO, err = d.grad_part(col0, n_local, lse32, max_pos)
        dv2, gO2, err2 = d.grad_part(col0, n_local, lse32, max_pos)
        assert err == 0 and err2 == 0
        assert np.array_equal(bits(dv), bits(dv2)) and np.array_equal(bits(gO), bits(gO2)), "second run differs in its bits"
        assert np.isnan(dv[B * c:]).all() and np.isnan(gO[n_local * c:]).all(), "written past an output"
        assert not (gO[:n_local * c] == -7.0).any(), "gO_local is not written in full"
        dv_sum = dv_sum + dv[:B * c].reshape(B, c)             # fp32, block order: what an all-reduce SUM does
        gO_rows.append(gO[:n_local * c].reshape(n_local, c))
    lse_ref, lse_bound = pc.merged_lse_reference(part, data)
    r_merge = cc._ratio(np.abs(pc.merge_lse(ms, ss) - lse_ref), lse_bound)
    ref_b = cc.stream_backward(case, data, lse32)
    r_dv, r_gO = cc.stream_backward_verdict(ref_b, dv_sum, np.concatenate(gO_rows, axis=0))
    print(f"[ce part] {part.name}: merged lse {r_merge:.4f}; dv shares summed {r_dv:.4f}, gO concatenated {r_gO:.4f} "
          f"(allowance 2)")
    assert r_merge <= 1.0 and r_dv <= 2.0 and r_gO <= 2.0


def test_ops_merge_lse_is_the_rule_of_the_cases(lib):
    """ops.ce_merge_lse on device tensors against ce_part_cases.merge_lse."""
    import r_tucker_amd as rt
    part = pc.PART_CASES[1]
    data, _, _ = setup(part.case)
    d = Device(lib, part.case, data)
    B = part.case.B
    got = [d.rows_part(a, n) for a, n in part.blocks]
    ms, ss = [g[0][:B] for g in got], [g[1][:B] for g in got]
    ms.append(np.full(B, -np.inf, dtype=np.float32))            # a block without rows
    ss.append(np.zeros(B))
    lse = rt.ce_merge_lse([dev(x) for x in ms], [dev(x) for x in ss])
    assert lse.dtype == torch.float64
    ref = pc.merge_lse(ms[:-1], ss[:-1])
    assert np.abs(lse.cpu().numpy() - ref).max() <= 2.0 ** -50 * (1.0 + np.abs(ref).max())
