"""Stage 1 (csrc/rtk_query.hip) element-wise against float64, for fp32 and bf16 operands.

The parameters are rounded to bf16 once, so the fp32 and the bf16 entry points see the same values and the
float64 reference (oracle.query_vectors_exact) is exact for both.  Stage 1 is two steps, the relation tables
T_u = G x_0 R[u] (b x c per relation) and the contraction v_d = S[h_d] . T_{r_d}; both sum in fp32.  With
u = 2^-24 and a factor two of slack, element-wise:
    tables   |dT| <= (a + 1) * 2^-23 * T_abs                         T_abs = |G| x_0 |R[u]|
    vectors  |dv| <= (a + b + 2) * 2^-23 * v_abs                     v_abs = query_vectors_exact(|G|, |R|, |S|)
for the VALU tables kernel (a <= 32, fmaf chains over a) and the bf16 MFMA tables (a > 32: the bf16 score kernel
with K = a, exact products, fp32 sums of ceil(a / 16) k-steps).
One path rounds more: fp32 operands with a > 32 build the tables on the split-fp16 GEMM (rtk_gemm_sf16_splitk,
operands split into fp16 halves scaled by the absolute maxima of ALL of R and G), whose bound
tests/test_gpu_round2.py::test_gemm_split_fp16_against_float64 states:
    tables   |dT| <= 2^-19 * T_abs + a * 2^-37 * max|R| * max|G|
    vectors  |dv| <= 2^-19 * v_abs + a * 2^-37 * max|R| * max|G| * sum_b |S[h_d]|  +  (b + 1) * 2^-23 * v_abs
Reference path replaced: src/model/asymmetric/R_TuckER.py:43-46.
"""
import numpy as np
import pytest
import torch

import gen
from oracle import score_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


CASES = [
    # (n_ent, n_rel, B, (a, b, c))    tables: fp32 / bf16 operands;  contraction
    (3000, 22, 96, (10, 64, 64)),     # VALU tables, vector loads (bc % 4 == 0);  per-query contract, vector loads
    (900, 22, 96, (7, 31, 31)),       # VALU tables, scalar loads (odd b c);  per-query contract, scalar loads
    (1500, 300, 64, (6, 48, 48)),     # VALU tables of a planned batch (n_rel > B: one slot per distinct relation)
    (900, 11, 2100, (8, 64, 64)),     # VALU tables;  grouped contract (B >= 2048)
    (1200, 40, 80, (64, 64, 64)),     # a > 32: split-fp16 GEMM / bf16 MFMA tables (KS = 4)
    (2000, 37, 256, (96, 128, 128)),  # a > 32: split-fp16 GEMM / bf16 MFMA tables (KS = 6)
    (900, 50, 2100, (40, 64, 64)),    # a > 32 tables;  grouped contract
    (600, 30, 2100, (300, 64, 64)),   # a > 256: bf16 MFMA tables at KS = 19 (the score kernel's deep-K instantiations)
    (2000, 300, 64, (272, 200, 200)), # a > 256, planned batch: the per-batch build (64 slots) runs the 4-wave form,
                                      # the all-relations build (300 slots x 40 000 (b, c) pairs) the 8-wave form
]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_stage1_against_float64(rt, case, dt):
    n_ent, n_rel, B, (a, b, c) = case
    core, R, S, _ = [torch.from_numpy(x).bfloat16() for x in gen.make_params(n_ent, n_rel, (a, b, c), 17)]
    h, r = [torch.from_numpy(x) for x in gen.make_queries(n_ent, n_rel, B, 17)]
    G64, R64, S64 = [x.double().numpy() for x in (core, R, S)]
    T64 = np.tensordot(R64, G64, axes=(1, 0))
    T_abs = np.tensordot(np.abs(R64), np.abs(G64), axes=(1, 0))
    v64 = orc.query_vectors_exact(G64, R64, S64, h, r)
    v_abs = orc.query_vectors_exact(np.abs(G64), np.abs(R64), np.abs(S64), h, r)
    sf16 = dt == torch.float32 and a > 32
    if sf16:
        floor = a * 2.0 ** -37 * np.abs(R64).max() * np.abs(G64).max()
        t_bound = 2.0 ** -19 * T_abs + floor
        v_bound = (2.0 ** -19 + (b + 1) * 2.0 ** -23) * v_abs + floor * np.abs(S64[h]).sum(1)[:, None]
    else:
        t_bound = (a + 1) * 2.0 ** -23 * T_abs
        v_bound = (a + b + 2) * 2.0 ** -23 * v_abs
    d = [x.to(dt).cuda() for x in (core, R, S)]
    hd, rd = h.cuda(), r.cuda()
    tables = rt.relation_tables(d[0], d[1])
    v0 = rt.query_vectors(*d, hd, rd)
    v1 = rt.query_vectors(*d, hd, rd, tables=tables)
    torch.cuda.synchronize()
    path = "split-fp16 GEMM" if sf16 else ("VALU" if a <= 32 else "bf16 MFMA")
    t_err = np.max(np.abs(tables.cpu().double().numpy() - T64) / t_bound)
    e0 = np.max(np.abs(v0.cpu().double().numpy() - v64) / v_bound)
    e1 = np.max(np.abs(v1.cpu().double().numpy() - v64) / v_bound)
    print(f"a={a} b={b} B={B} n_rel={n_rel} {dt}: {path} tables {t_err:.2e}, vectors {e0:.2e}, from tables {e1:.2e}"
          " (max error / bound)")
    assert t_err <= 1.0, "relation tables"
    assert e0 <= 1.0, "query vectors"
    assert e1 <= 1.0, "query vectors from the tables"
