"""The ordered scatter through rtk_score_candidates_bwd_f32 (dv = NULL), bit for bit against the float32 emulation of
tests/golden/scatter_cases.py: the stable sort by entity, the windowed run sums and the combine of the runs that cross
windows.  The operands carry 12 significant bits, so the kernels' fmaf chain is a chain of float32 adds and gO has
to equal the emulation exactly; a change of window, of the order inside a run or of the combine order changes the
bits (tests/test_scatter_cases_host.py proves that on the host).

Every call: gO inside a NaN-filled buffer with guards in front of it and behind it, the workspace pre-filled with
0xFF, O all NaN (gO never reads O), the padding of dz a sentinel.  No tolerances.
"""
import numpy as np
import pytest
import torch

import scatter_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 64
by_name = dict(ids=lambda c: c.name)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def dev(a):
    t = torch.from_numpy(np.array(a, order="C")).cuda()                     # a copy: the cases' operands are read-only
    assert t.data_ptr() % 16 == 0
    return t


def run(lib, case, bf16=False):
    """-> gO (n_ent, c) as the entry left it; checks the floats in front of it and behind it."""
    cand, dz, v = sc.operands(case)
    B, K, c, N = case.B, case.K, case.c, case.n_ent
    d_cand = dev(cand if cand.size else np.zeros(1, np.int64))
    d_dz = dev(dz if dz.size else np.zeros(1, np.float32))
    d_v = dev(np.concatenate([np.zeros(4 + case.v_off, np.float32), v.reshape(-1)]))
    v_ptr = d_v.data_ptr() + 4 * (4 + case.v_off)
    O = torch.full((N, c), float("nan"), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    front = 4 + case.go_off
    buf = torch.full((front + N * c + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    g_ptr = buf.data_ptr() + 4 * front
    assert (v_ptr % 16 == 0) == (case.v_off % 4 == 0) and (g_ptr % 16 == 0) == (case.go_off % 4 == 0)
    nws = int(lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N))
    assert (nws == 0) == (case.M == 0)
    ws = torch.full((max(nws, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    before = buf.cpu().numpy()
    fn = lib.rtk_score_candidates_bwd_bf16 if bf16 else lib.rtk_score_candidates_bwd_f32
    rc = fn(d_dz.data_ptr(), K + case.dz_pad, v_ptr, B, c, O.data_ptr(), N, d_cand.data_ptr(),
            0 if case.shared else K + case.cand_pad, K, None, g_ptr, ws.data_ptr(), nws,
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.array_equal(bits(h[:front]), bits(before[:front])), "written in front of gO"
    assert np.array_equal(bits(h[front + N * c:]), bits(before[front + N * c:])), "written past gO"
    return h[front:front + N * c].reshape(N, c)


def first_difference(got, ref):
    bad = np.argwhere(bits(got) != bits(ref))
    i = tuple(bad[0])
    return f"{len(bad)} of {ref.size} elements differ; first at {i}: got {got[i]!r}, expected {ref[i]!r}"


@pytest.mark.parametrize("case", sc.CASES, **by_name)
def test_gO_bits(lib, case):
    got, ref = run(lib, case), sc.expected(case)
    assert np.array_equal(bits(got), bits(ref)), f"[{case.name}] " + first_difference(got, ref)


def test_gO_bits_with_bf16_operands(lib):
    case = sc.BY_NAME[sc.BF16_CASE]
    got, ref = run(lib, case, bf16=True), sc.expected(case)
    assert np.array_equal(bits(got), bits(ref)), f"[{case.name}, bf16] " + first_difference(got, ref)
