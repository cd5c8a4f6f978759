"""Host checks of tests/golden/split_cases.py, the numpy model of the split-fp16 score kernels and the operands on which it
is exact (no GPU): the exactness criterion of every case, fp32 accumulation in random orders, the fifth group's cut, the
mutants (each must change an output of a case on every shape it applies to; printed) and the real layer's split bound."""
import os
import subprocess

import numpy as np
import pytest

import split_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from r_tucker_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):   # build in-tree (hipcc cross-compiles gfx950 without a GPU)
        subprocess.run(["bash", os.path.join(ROOT, "r-tucker_amd", "csrc", "build.sh")], check=True)
    return _lib.load()


def fifth_mask(lib, shape, hint):
    """fifth-group columns of the kernel that runs on `shape` under `hint` (0 on a shape the cg kernel does not cover)"""
    mask = np.zeros(shape.N, dtype=np.uint8)
    if "cg" in shape.kernels:
        assert lib.rtk_score_fifth_group_columns_f32(shape.N, shape.c, hint, mask.ctypes.data) >= 0
    return mask.view(bool)


def test_pack_shift_rule():
    f = lambda x: int(sc.pack_shift(F32(x)))
    assert [f(16384.0), f(32767.0), f(32768.0), f(1.0), f(0.75), f(2.0 ** -80)] == [0, 0, -1, 14, 15, 94]
    assert f(np.nextafter(F32(16384.0), F32(0))) == 1
    assert f(2.0 ** -86) == 100 and f(2.0 ** -87) == 100 and f(2.0 ** -149) == 100          # the clamp
    assert f(2.0 ** 114) == -100 and f(2.0 ** 115) == -100 and f(3.0e38) == -100
    assert f(0.0) == 0 and f(-1.0) == 0 and f(np.inf) == 0 and f(np.nan) == 0
    hi, lo, sh = sc.split(np.array([[3.0, -1.0 - 2.0 ** -12, 0.0]], dtype=F32))
    assert sh[0] == 13 and hi[0].tolist() == [24576.0, -8192.0, 0.0] and lo[0].tolist() == [0.0, -2.0, 0.0]
    # a global bound in place of the row maximum
    assert sc.split(np.ones((2, 3), dtype=F32), bound=4.0)[2].tolist() == [12, 12]


def test_shapes_cover_the_kernels_branches():
    S = sc.SHAPES
    v3_only = [s for s in S if s.kernels == ("v3",)]
    assert {sc.ksteps(s.c) for s in S if s.N < 1000} >= {1, 13, 14, 16, 17, 32}
    assert {s.B for s in S if s.N < 1000} >= {1, 33, 70}
    assert {s.c for s in v3_only} >= {36, 200, 7, 97, 509}
    assert any(s.o_off and s.c % 4 == 0 for s in S)
    assert any(-(-s.N // 128) * -(-s.B // 32) > 512 and s.c == 16 for s in S)
    assert {s.N % 128 for s in S} >= {0, 1, 127}
    assert any(s.N < 32 for s in S) and any(s.N >= 32768 for s in S) and any(s.pitch and s.pitch * 4 % 128 == 0 for s in S)
    # tail: where the maximal element sits, for every c % 16 class in use
    for c in {s.c for s in S}:
        pos = sc._tail_positions(c)
        assert pos[:2] == [c - 1, 0]
        if c % 16 == 0 or c % 16 > 8:
            assert len(pos) == 3 and pos[2] // 16 == sc.ksteps(c) - 1 and pos[2] % 16 >= 8 and pos[2] < c
        elif c > 8:
            assert len(pos) == 3 and pos[2] // 16 == sc.ksteps(c) - 2 and pos[2] % 16 >= 8


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_exact_cases_hold_and_catch_the_mutants(lib, shape):
    rng = np.random.default_rng(5)
    masks = {h: fifth_mask(lib, shape, h) for h in (0, 0x100)}
    for family in sc.FAMILIES:
        case = sc.make_case(shape, family)
        m, head = sc.assert_exact(case, case.model)
        P = case.P
        ok = case.valid if case.valid is not None else np.ones(m.z.shape, dtype=bool)
        # fp32 accumulation of the 3 c products, three random orders, a sample of outputs
        dd, jj = np.nonzero(ok)
        pick = rng.choice(dd.size, size=min(48, dd.size), replace=False)
        for d, j in zip(dd[pick], jj[pick]):
            prods = np.concatenate([P.vh[d] * P.oh[j], P.vh[d] * P.ol[j], P.vl[d] * P.oh[j]])
            p32 = prods.astype(F32)
            assert np.array_equal(p32.astype(F64), prods)
            for _ in range(3):
                s = np.cumsum(rng.permutation(p32), dtype=F32)[-1]
                assert F64(s) == m.acc[d, j], (case.name, d, j)
                z = F32(F32(s) * F32(2.0) ** F32(-m.shv[d])) * F32(2.0) ** F32(-m.sho[j])      # (acc * sv) * us_o
                assert F64(z) == m.z[d, j], (case.name, d, j)
        # the fifth group's cut cannot change a bit
        for h, mask in masks.items():
            if mask.any():
                assert np.array_equal(sc.accumulate(P, mask), m.acc), (case.name, h)
        lo_both = float(np.mean((P.vl != 0).any(axis=1))), float(np.mean((P.ol != 0).any(axis=1)))
        print(f"{case.name}: max T / g = 2^{np.log2(head):.2f}; rows with a non-zero lo: v {lo_both[0]:.2f}, O {lo_both[1]:.2f}; "
              f"|z| {np.abs(m.z[ok][m.z[ok] != 0]).min():.2e} .. {np.abs(m.z[ok]).max():.2e}"
              + (f"; outputs kept {ok.mean():.2f}" if case.valid is not None else ""))
        if family == "fewbit":
            both = np.mean((P.vl != 0)[P.vh != 0]), np.mean((P.ol != 0)[P.oh != 0])
            assert min(both) > 0.6, "both lo planes populated"
            if shape.N * shape.B >= 20000:       # the logistic's whole range, saturation on both sides
                assert m.z.min() < -104 and m.z.max() > 18 and np.abs(m.z[m.z != 0]).min() < 2.0 ** -6
        if family == "scale":
            ev, eo = 14 - m.shv, 14 - m.sho
            kept = {(a, b) for a in sc.SCALE_EXPS for b in sc.SCALE_EXPS if ok[np.ix_(ev == a, eo == b)].all()
                    and (ev == a).any() and (eo == b).any()}
            if shape.B >= 5:
                assert (-60, -40) in kept and (60, 60) in kept and (-60, -60) not in kept
        if family == "sublo":
            lo = np.concatenate([np.abs(P.vl[P.vl != 0]), np.abs(P.ol[P.ol != 0])])
            assert lo.max() <= 2.0 ** -14, "every non-zero lo is an fp16 subnormal (or, rounded up, the smallest normal number)"
        check_mutants(case, masks[0x100])


def check_mutants(full, mask):
    """every mutant that `full`'s family has to catch changes an output (of a window of the case: mutants are local)"""
    full.fifth = mask
    for name, (fn, family, applies) in sc.MUTANTS.items():
        if family != full.family:
            continue
        if not applies(full):
            print(f"{full.shape.id}: '{name}' does not apply")
            continue
        case = sc.window(full)
        good = sc.score_model(case.v, case.O, case.fifth).z
        with np.errstate(over="ignore", invalid="ignore"):
            bad = fn(case)
        ok = case.valid if case.valid is not None else np.ones(good.shape, dtype=bool)
        changed = int(((bad != good) & ok).sum())
        print(f"{full.shape.id}: '{name}' changes {changed} of {int(ok.sum())} outputs of {case.name}")
        assert changed > 0, f"'{name}' is not caught by {case.name}"
    full.fifth = None


def test_every_mutant_has_a_family_that_runs_on_every_shape():
    assert {family for _, family, _ in sc.MUTANTS.values()} <= set(sc.FAMILIES) and len(sc.MUTANTS) == 15


@pytest.mark.parametrize("kind", ["rows", "range"])
@pytest.mark.parametrize("shape", [s for s in sc.SHAPES if s.N <= 4100], ids=[s.id for s in sc.SHAPES if s.N <= 4100])
def test_real_layer_stays_inside_the_split_bound(shape, kind):
    case = sc.real_case(shape, kind)
    m, bound = sc.split_bound(case.v, case.O)
    z64 = case.v.astype(F64) @ case.O.astype(F64).T
    T64 = np.abs(case.v).astype(F64) @ np.abs(case.O).astype(F64).T
    ratio = np.abs(m.z - z64) / (bound + 2.0 ** -50 * T64)         # (the float64 products' own rounding)
    print(f"{case.name}: max |z_model - z64| / bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    # ... and the header's normwise statement follows.  Per k: 2^-11 ulp_fp16(hi) <= 2^-7 against an element below 2^15,
    # on either side (2^9), and |vl| |ol| <= 2^3 2^3, over max max >= 2^28:  (2^-19 + 2^-22) c max|v_d| max|O_j|
    nb = (2.0 ** -19 + 2.0 ** -22 + 2.0 ** -30) * shape.c * np.abs(case.v).max(axis=1).astype(F64)[:, None] * np.abs(case.O).max(axis=1).astype(F64)[None, :]
    assert (bound <= nb).all()
