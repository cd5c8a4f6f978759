"""The method of tests/test_gpu_ce_kernels.py, proved without a GPU on the cases of tests/golden/ce_kernel_cases.py:

  * fp32 numpy emulations of ce_rows_kernel, of the two gradient passes and of the matrix-free backward's link stay
    within the derived bounds on every case, also with every exponential moved one ulp up or down (the hardware's exp2
    is not correctly rounded);
  * every named mutant -- a kernel that is wrong in one way -- is outside the bound on at least one case, judged by the
    verdict functions the GPU tests use: no bound is vacuous;
  * the conditions the derivation states hold: family E's logits are exact, every forward case has a row whose maximum
    is in the last valid column, family G's bounds leave the lo planes visible, the floors stay small.
"""
import functools

import numpy as np
import pytest

import ce_kernel_cases as cc


@functools.lru_cache(maxsize=None)
def rows_setup(case):
    csr, Z = cc.setup_rows(case)
    lse, _ = cc.rows_reference(case, Z, csr)
    return csr, Z, lse.astype(np.float32)


@functools.lru_cache(maxsize=None)
def stream_setup(case):
    data = cc.stream_operands(case)
    fwd = cc.stream_forward(case, data)
    lse32 = fwd[0].astype(np.float32)
    return data, fwd, lse32, cc.stream_backward(case, data, lse32)


by_name = dict(ids=lambda c: c.name)


# ------------------------------------------------------------------------------------- emulations pass ----
@pytest.mark.parametrize("perturb", [0, 1, -1])
@pytest.mark.parametrize("case", cc.ROWS_CASES + [cc.CHAINED_CASE], **by_name)
def test_rows_emulation_within_bounds(case, perturb):
    csr, Z, _ = rows_setup(case)
    lse, rows = cc.emul_rows(case, Z, csr, perturb)
    r_lse, r_rows = cc.rows_verdict(case, Z, csr, lse, rows)
    print(f"\n[ce rows, emulated] {case.name} {perturb:+d}: error / bound = {r_lse:.4f} (lse_out), {r_rows:.4f} (rows)")
    assert r_lse <= 1.0 and r_rows <= 1.0


@pytest.mark.parametrize("perturb", [0, 1, -1])
@pytest.mark.parametrize("case", cc.GRAD_CASES, **by_name)
def test_grad_emulation_within_bounds(case, perturb):
    csr, Z, lse32 = rows_setup(case)
    r = cc.grad_verdict(case, Z, csr, lse32, cc.emul_grad(case, Z, csr, lse32, perturb))
    print(f"\n[ce grad, emulated] {case.name} {perturb:+d}: error / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("perturb", [0, 1, -1])
@pytest.mark.parametrize("case", cc.STREAM_CASES, **by_name)
def test_stream_link_emulation_within_bounds(case, perturb):
    data, _, lse32, ref = stream_setup(case)
    dv, gO = cc.emul_stream_grad(case, data, lse32, perturb)
    r_dv, r_gO = cc.stream_backward_verdict(ref, dv, gO)
    print(f"\n[ce stream, emulated link] {case.name} {perturb:+d}: error / bound = {r_dv:.4f} (dv), {r_gO:.4f} (gO)")
    assert r_dv <= 1.0 and r_gO <= 1.0


def test_the_float64_references_pass_their_own_verdicts():
    for case in cc.ROWS_CASES[:3]:
        csr, Z, lse32 = rows_setup(case)
        lse, rows = cc.rows_reference(case, Z, csr)
        assert max(cc.rows_verdict(case, Z, csr, lse32, rows)) <= 1.0
    for case in cc.STREAM_CASES[-3:]:
        data, fwd, lse32, ref = stream_setup(case)
        assert max(cc.stream_forward_verdict(fwd, lse32, fwd[1])) <= 1.0
        assert max(cc.stream_backward_verdict(ref, ref["dv"].astype(np.float32), ref["gO"].astype(np.float32))) <= 1.0


# ------------------------------------------------------------------------------------- mutants fail -------
ROWS_MUTANTS = ["drop_last_column", "duplicate_last_column", "no_rescale", "no_t0", "w_one_on_empty", "wrap_ids",
                "count_in_range", "first_256_only"]


@pytest.mark.parametrize("mutant", ROWS_MUTANTS)
def test_rows_mutant_fails(mutant):
    failed = []
    for case in cc.ROWS_CASES:
        csr, Z, _ = rows_setup(case)
        if mutant == "no_rescale":
            lse, rows = cc.emul_rows(case, Z, csr, rescale=False)
        else:
            lse, rows = cc.rows_reference(case, Z, csr, mutant)
        if max(cc.rows_verdict(case, Z, csr, lse.astype(np.float32), rows)) > 1.0:
            failed.append(case.name)
    print(f"\n[ce rows] mutant {mutant} fails {failed}")
    assert failed


GRAD_MUTANTS = ["no_t0", "first_64_only", "once_per_slot_user", "neighbour_w", "neighbour_lse", "padding_written"]


@pytest.mark.parametrize("mutant", GRAD_MUTANTS)
def test_grad_mutant_fails(mutant):
    failed = []
    for case in cc.GRAD_CASES[:-1]:                          # (the capped case adds nothing to the proof)
        csr, Z, lse32 = rows_setup(case)
        full = Z.copy()
        with np.errstate(over="ignore", invalid="ignore"):   # a neighbour's lse may overflow the exponential
            full[:, :case.N] = cc.grad_reference(case, Z, csr, lse32, None if mutant == "padding_written" else mutant)
        if mutant == "padding_written":
            full[:, case.N:] = 0.0
        if cc.grad_verdict(case, Z, csr, lse32, full) > 1.0:
            failed.append(case.name)
    print(f"\n[ce grad] mutant {mutant} fails {failed}")
    assert failed


STREAM_MUTANTS = ["query_past_B", "column_past_N", "x_lo_dropped", "O_lo_dropped", "sv_lo_dropped",
                  "scatter_slot_minus_one", "merge_without_split_maximum"]


@pytest.mark.parametrize("mutant", STREAM_MUTANTS)
def test_stream_mutant_fails(mutant):
    failed = []
    for case in cc.SHAPE_CASES:
        if mutant in ("O_lo_dropped", "sv_lo_dropped") and case.family != "G":
            continue
        data, fwd, lse32, ref = stream_setup(case)
        if mutant == "merge_without_split_maximum":
            lse, rows = cc.stream_forward(case, data, mutant)[:2]
            bad = max(cc.stream_forward_verdict(fwd, lse.astype(np.float32), rows)) > 1.0
        else:
            m = cc.stream_backward(case, data, lse32, mutant)
            r_dv, r_gO = cc.stream_backward_verdict(ref, m["dv"].astype(np.float32), m["gO"].astype(np.float32))
            bad = (r_dv if mutant in ("column_past_N", "O_lo_dropped") else
                   r_gO if mutant in ("query_past_B", "sv_lo_dropped", "scatter_slot_minus_one") else max(r_dv, r_gO)) > 1.0
        if bad:
            failed.append(case.name)
    print(f"\n[ce stream] mutant {mutant} fails {failed}")
    assert failed


def test_a_nonzero_dv_row_of_mass_zero_is_refused():
    case = next(c for c in cc.SHAPE_CASES if c.eps == 0.0)
    data, _, _, ref = stream_setup(case)
    assert (ref["w"] == 0.0).sum() >= 2, "eps = 0: the empty list and the row without a list have no mass"
    dv = ref["dv"].astype(np.float32)
    dv[np.nonzero(ref["w"] == 0.0)[0][0], 0] = np.float32(-0.0)
    assert cc.stream_backward_verdict(ref, dv, ref["gO"].astype(np.float32))[0] == np.inf


# ------------------------------------------------------------------------------------- stated conditions --
def test_csr_conventions():
    for case in cc.ROWS_CASES + cc.GRAD_CASES:
        csr, _, _ = rows_setup(case)
        assert csr.slot[case.B - 1] == 0
        if case.B >= 18:
            assert (csr.slot == -1).sum() == 1
            assert np.bincount(csr.slot[csr.slot >= 0]).min() >= 2, "several rows share every slot"
        for s, n in enumerate(case.lengths):
            l = csr.obj[csr.ptr[s]:csr.ptr[s + 1]]
            if n >= 6:
                assert {-1, case.N, case.N + 5} <= set(l.tolist())
            good = l[(l >= 0) & (l < case.N)]
            assert len(set(good.tolist())) == len(good)
    assert any(max(c.lengths) > 256 for c in cc.ROWS_CASES) and any(max(c.lengths) > 64 for c in cc.GRAD_CASES)
    for case in cc.SHAPE_CASES:
        csr = stream_setup(case)[0].csr
        users = np.zeros(case.N, dtype=int)
        for d in range(case.B):
            users[csr.positives(d, case.N)] += 1
        if case.B >= 70:
            assert users[0] >= 40 and users[case.N - 1] >= 40, "a positive shared by at least 40 queries"
        if case.B > 1:
            assert (csr.slot == -1).sum() == 1 and csr.longest() > min(128, case.N)    # (unique objects: at most N + 3)


def test_every_forward_case_has_a_row_maximum_in_the_last_valid_column():
    for case in cc.ROWS_CASES + [cc.CHAINED_CASE]:
        _, Z, _ = rows_setup(case)
        assert (np.argmax(Z[:, :case.N], axis=1) == case.N - 1).any(), case.name
        assert np.isnan(Z[:, case.N:]).all()
    for case in cc.STREAM_CASES:
        z = stream_setup(case)[0].z
        last = z[:, case.N - 1]
        assert case.N == 1 or (last > np.delete(z, case.N - 1, axis=1).max(axis=1)).any(), case.name


def test_family_e_logits_are_exact():
    for case in cc.STREAM_CASES:
        if case.family != "E":
            continue
        data = stream_setup(case)[0]
        v, O = data.v.astype(np.float64), data.O.astype(np.float64)
        q = np.abs(v[v != 0]).min()
        iv = v / q
        assert np.array_equal(iv, np.round(iv)) and np.abs(iv).max() <= 2 and np.log2(q) == np.round(np.log2(q))
        assert np.array_equal(O, np.round(O)) and np.abs(O).max() <= 2
        # one significant bit per operand: hi is the value, lo = 0; every partial sum is an integer multiple of q below
        # 2^24 q, exact in fp32 in any order; the row and column factors are powers of two
        assert (np.abs(iv).sum(axis=1).max() * 2) < 2 ** 24
        assert np.array_equal(v.astype(np.float16).astype(np.float64) * 1.0, v) or np.abs(v).max() >= 2.0 ** 15
        assert np.array_equal(data.z.astype(np.float32).astype(np.float64), data.z)
        if case.B * case.N >= 3000:
            assert 2.0 <= data.z.std() <= 3.0, (case.name, data.z.std())


def test_family_g_scales():
    for case in cc.STREAM_CASES:
        if case.family == "G" and case.B * case.N >= 1000:
            z = stream_setup(case)[0].z
            assert 0.8 * case.sigma <= z.std() <= 1.25 * case.sigma, (case.name, z.std())
    assert any(c.sigma == 25.0 for c in cc.STREAM_CASES)


@pytest.mark.parametrize("case", [c for c in cc.STREAM_CASES if c.family == "G"], **by_name)
def test_family_g_bounds_leave_the_lo_planes_visible(case):
    """No per-element bound of the sweep above 2^-13 sum |x| |O| (the floor and the roundings of the positives' own
    share, which no lo plane enters, aside); kappa as derived."""
    data, _, _, ref = stream_setup(case)
    r_dv = (ref["dv_sweep"] / np.maximum(ref["dv_mass"], 1e-300)).max()
    r_gO = (ref["gO_sweep"] / np.maximum(ref["gO_mass"], 1e-300)).max()
    print(f"\n[ce stream] {case.name}: sweep bound / sum|x||O| <= {r_dv * 2 ** 13:.3f} (dv), {r_gO * 2 ** 13:.3f} (gO) x 2^-13")
    assert r_dv <= 2.0 ** -13 and r_gO <= 2.0 ** -13
    S = np.abs(data.v.astype(np.float64)) @ np.abs(data.O.astype(np.float64)).T
    assert np.all(cc.chain_bound(case, data) <= (3 + 0.75 * case.ks) * 1.01 * cc.U22 * S)


@pytest.mark.parametrize("case", cc.STREAM_CASES, **by_name)
def test_floors_stay_small(case):
    """The floor is more than half of an element's bound for at most 5 % of the elements (rows of mass w_d = 0, whose
    dv is asserted to be zero bit for bit, aside)."""
    _, _, _, ref = stream_setup(case)
    live = ref["w"] > 0
    f_dv = (ref["dv_floor"][live] > 0.5 * ref["dv_b"][live]).mean() if live.any() else 0.0
    f_gO = (ref["gO_floor"] > 0.5 * ref["gO_b"]).mean()
    assert f_dv <= 0.05 and f_gO <= 0.05, (f_dv, f_gO)


def test_case_lists_cover_the_branches():
    assert sorted(c.c // 16 for c in cc.KS_CASES) == list(range(1, 14))
    assert {c.N for c in cc.ROWS_CASES} == {1, 255, 257, 2047, 2048, 2049, 4097, 5889}
    assert any(c.B == 70 for c in cc.ROWS_CASES) and any(c.pad for c in cc.ROWS_CASES)
    assert {c.eps for c in cc.ROWS_CASES} == {0.0, 0.1}
    assert sorted(c.N % 4 for c in cc.GRAD_CASES[:4]) == [0, 1, 2, 3] and all(c.ld % 4 == 0 for c in cc.GRAD_CASES[:4])
    assert cc.GRAD_CASES[4].ld % 4 == 1 and cc.GRAD_CASES[5].off == 1 and cc.GRAD_CASES[5].ld % 4 == 0
    assert -(-270339 // 4096) > 64                            # the capped grid strides twice
    assert sum(c.eps == 0.0 for c in cc.SHAPE_CASES) == 2
    # B = 129: two query groups -> 128 splits over 94 tiles: splits without a tile inside the range
    e = cc.split_edges(129, 3003)
    assert len(e) == 129 and e[-1] == 94 and any(a == b for a, b in zip(e[1:-2], e[2:-1]))
    assert cc.splits_of(513) == 51 and cc.split_edges(513, 257)[-1] == 9
