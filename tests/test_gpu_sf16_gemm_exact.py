"""The split-fp16 GEMM (rtk_gemm_sf16_splitk) through the C ABI, bit for bit against the numpy split model of
tests/golden/sf16_gemm_cases.py, and rtk_absmax_f32 against np.abs(x).max() exactly.

The exact cases are operands on which the model cannot round (tests/test_sf16_gemm_cases_host.py proves that, and that
seventeen mutants of the model are visible, on the host), so the kernel has to return the model whatever its summation
order: on the four (a_kmajor, b_kmajor) instantiations, with 16-byte and 4-byte K-major loads, at every fragment edge of
K, through clamped rows, the tile remap and split-K.  Every case: GARBAGE around the operands (nan and inf bit patterns
behind a K-major row, huge finite values around an M-major operand), C pre-filled with a sentinel that must survive in
front of C, in the columns [N, ldc) and past row M, the workspace pre-filled with 0xFF bytes, a second launch
bit-identical.  A real-valued layer is held to gamma(3 K_chunk + splits) T around the model.
"""
import numpy as np
import pytest
import torch

import sf16_gemm_cases as gc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = -777.25          # not an integer multiple of any case's unit
GUARD = 64                  # floats in front of and behind C that must keep the sentinel
RTK_ERR_BAD_ARG, RTK_ERR_WORKSPACE = -1, -2
_cases = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    return r_tucker_amd._lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def case_of(shape, family):
    key = (shape.id, family)
    if key not in _cases:
        _cases[key] = gc.make_case(shape, family)
    return _cases[key]


class Operand:
    """an operand on the device in one layout, with garbage around it"""
    def __init__(self, X, kmajor, shape):
        pad, off = shape.pad_off(kmajor, X.shape[1] if kmajor else X.shape[0])
        flat, off, self.ld = gc.lay_out(X, kmajor, pad, off)
        self.t = torch.from_numpy(flat).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr, self.kmajor = self.t.data_ptr() + 4 * off, kmajor
        assert not kmajor or ((self.ptr % 16 == 0 and self.ld % 4 == 0) == (shape.mode == "vec"))


def scalar(x):
    return torch.from_numpy(np.array([x], dtype=F32)).cuda()


def launch(lib, shape, a, b, ba, bb, splits=None, ws_bytes=None, ldc=None):
    """one call on fresh C and workspace -> (rc, the whole C buffer on the host, ldc)"""
    M, N, K = shape.M, shape.N, shape.K
    splits = shape.splits if splits is None else splits
    ldc = N + shape.ldc_pad if ldc is None else ldc
    buf = torch.full((GUARD + shape.c_off + M * (N + shape.ldc_pad) + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    need = lib.rtk_gemm_f32_splitk_workspace_bytes(M, N, splits) if splits > 1 else 0
    ws = torch.full((max(need, 256),), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.rtk_gemm_sf16_splitk(a.ptr, a.kmajor, a.ld, ba.data_ptr() if ba is not None else None, b.ptr, b.kmajor, b.ld,
                                  bb.data_ptr() if bb is not None else None, buf.data_ptr() + 4 * (GUARD + shape.c_off), ldc,
                                  M, N, K, splits, ws.data_ptr() if splits > 1 else None,
                                  (need if ws_bytes is None else ws_bytes) if splits > 1 else 0, _stream())
    torch.cuda.synchronize()
    return rc, buf.cpu().numpy(), ldc


def read_c(shape, h, ldc):
    """the M x N result; everything around it still holds the sentinel"""
    M, N, c0 = shape.M, shape.N, GUARD + shape.c_off
    body = h[c0:c0 + M * ldc].reshape(M, ldc)
    assert np.all(h[:c0] == SENTINEL), "written in front of C"
    assert np.all(h[c0 + M * ldc:] == SENTINEL), "written past row M"
    assert np.all(body[:, N:] == SENTINEL), "written in the columns [N, ldc)"
    return body[:, :N].copy()


def run_twice(lib, shape, a, b, ba, bb):
    outs = []
    for _ in range(2):
        rc, h, ldc = launch(lib, shape, a, b, ba, bb)
        assert rc == 0, lib.rtk_last_error_string()
        outs.append(read_c(shape, h, ldc))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "second launch differs in its bits"
    return outs[0]


def operands(case, layouts=gc.LAYOUTS):
    """the case's operands in each layout (every storage uploaded once)"""
    A = {k: Operand(case.A, k, case.shape) for k in {ak for ak, _ in layouts}}
    B = {k: Operand(case.B, k, case.shape) for k in {bk for _, bk in layouts}}
    ba, bb = scalar(case.ba), scalar(case.bb)
    for ak, bk in layouts:
        yield (ak, bk), A[ak], B[bk], ba, bb


def differences(got, ref, ok):
    bad = np.argwhere((got.astype(F64) != ref.astype(F64)) & ok)
    if len(bad) == 0:
        return ""
    i, j = bad[0]
    return f"{len(bad)} of {int(ok.sum())} outputs differ; first at ({i}, {j}): got {got[i, j]!r}, model {ref[i, j]!r}"


def check_exact(lib, case):
    m = case.model
    assert np.isfinite(m.C[case.valid]).all()
    for layout, a, b, ba, bb in operands(case):
        got = run_twice(lib, case.shape, a, b, ba, bb)
        d = differences(got, m.C, case.valid)
        assert not d, f"{case.name}, layout {layout}: {d}"


@pytest.mark.parametrize("shape", gc.SHAPES + [gc.LONG], ids=gc.SHAPE_IDS + [gc.LONG.id])
def test_gemm_equals_the_split_model(lib, shape):
    for family in (gc.FAMILIES_ALL_SHAPES if shape is not gc.LONG else ("hionly",)):
        check_exact(lib, case_of(shape, family))


@pytest.mark.parametrize("kind", ["bound", "scale"])
@pytest.mark.parametrize("shape", [gc.SMALL, gc.SMALL_SPLIT], ids=lambda s: s.id)
def test_gemm_bounds_and_scales_equal_the_split_model(lib, shape, kind):
    n = 0
    for family in gc.small_families():
        if family.startswith(kind):
            case = case_of(shape, family)
            if case is not None:
                check_exact(lib, case)
                n += 1
    assert n >= (24 if kind == "bound" else 40)


def test_gemm_positive_scales_equal_the_split_model(lib):
    cases = [c for c in (case_of(gc.POS_SHAPE, f) for f in gc.pos_families()) if c is not None]
    assert len(cases) >= 30
    for case in cases:
        check_exact(lib, case)


def test_control_the_device_output_differs_from_mutants(lib):
    """One launch per layout at M = 130, N = 70, K = 97: the output that equals the model differs from three mutants."""
    shape = gc.CONTROL
    for family, names in (("fewbit", ("al.bl added", "hi truncated")), ("bound:ratio1024:A", ("shift from the true maximum",))):
        case = case_of(shape, family)
        bad = {name: gc.MUTANTS[name][0](case) for name in names}
        for layout, a, b, ba, bb in operands(case):
            rc, h, ldc = launch(lib, shape, a, b, ba, bb)
            assert rc == 0
            got = read_c(shape, h, ldc)
            assert not differences(got, case.model.C, case.valid)
            for name, wrong in bad.items():
                n = int(((got != wrong) & case.valid).sum())
                print(f"\n[sf16 control] layout {layout}: differs from '{name}' in {n} of {got.size} entries, from the model in 0")
                assert n > 0


REAL_SHAPES = [gc.CONTROL, gc._s(129, 129, 64, 2), gc._s(70, 36, 515, 4, mode="odd"), gc._s(257, 33, 161, 1, mode="off"), gc.LONG]


@pytest.mark.parametrize("mag", [3e-9, 1.0, 1e20], ids=lambda m: f"mag{m:g}")
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: s.id)
def test_gemm_real_values_within_gamma_bound_of_the_model(lib, shape, mag):
    case = gc.real_case(shape, mag, 1.0)
    case.ba = F32(3 * case.ba)          # a loose caller bound, as the BCE gradient has it
    m = gc.gemm_model(gc.planes(case.A, case.B, case.ba, case.bb), shape.K, shape.splits)
    bound = gc.real_bound(m, shape.K, shape.splits)
    for layout, a, b, ba, bb in operands(case):
        got = run_twice(lib, shape, a, b, ba, bb)
        err = np.abs(got.astype(F64) - m.C64)
        ratio = float(np.max(err / np.maximum(bound, np.finfo(F64).tiny)))
        print(f"\n[sf16 real] {case.name} layout {layout}: max error / gamma bound = {ratio:.4f}")
        assert np.isfinite(got).all() and np.all(err <= bound), f"layout {layout}: max error / bound = {ratio}"


def test_gemm_nan_and_inf_stay_in_their_row_and_column(lib):
    shape = gc.CONTROL
    clean = gc.real_case(shape, 1.0, 1.0)
    i0, j0 = 67, 33
    A, B = clean.A.copy(), clean.B.copy()
    A[i0, 5], A[i0, shape.K - 1] = np.nan, np.inf
    B[j0, 0], B[j0, 40] = -np.inf, np.nan
    dirty = gc.Case("planted", "real", shape, A, B, clean.ba, clean.bb)
    outside = np.ones((shape.M, shape.N), dtype=bool)
    outside[i0, :] = False
    outside[:, j0] = False
    for (layout, a, b, ba, bb), (_, a2, b2, _, _) in zip(operands(clean), operands(dirty)):
        ref = run_twice(lib, shape, a, b, ba, bb)
        got = run_twice(lib, shape, a2, b2, ba, bb)
        assert np.isfinite(ref).all()
        assert np.array_equal(got.view(np.uint32)[outside], ref.view(np.uint32)[outside]), f"layout {layout}: leaked"
        assert not np.isfinite(got[~outside]).any(), f"layout {layout}: a finite output in the planted row or column"


def test_gemm_error_returns(lib):
    shape = gc.SMALL_SPLIT
    case = case_of(shape, "fewbit")
    (_, a, b, ba, bb), = operands(case, layouts=((1, 0),))
    need = lib.rtk_gemm_f32_splitk_workspace_bytes(shape.M, shape.N, shape.splits)
    assert need >= shape.M * shape.N * 4 * shape.splits

    def untouched(rc_h_ldc, rc):
        assert rc_h_ldc[0] == rc and np.all(rc_h_ldc[1] == SENTINEL)

    for given in (need - 1, 16, 0):
        untouched(launch(lib, shape, a, b, ba, bb, ws_bytes=given), RTK_ERR_WORKSPACE)
    wide = gc._s(shape.M, shape.N, shape.K, shape.splits, shape.mode, ldc_pad=1)
    untouched(launch(lib, wide, a, b, ba, bb), RTK_ERR_BAD_ARG)                      # ldc != N with splits > 1
    rc, h, ldc = launch(lib, wide, a, b, ba, bb, splits=1)                           # ... is what splits == 1 takes
    assert rc == 0 and not differences(read_c(wide, h, ldc), gc.gemm_model(case.P, shape.K, 1).C, case.valid)
    untouched(launch(lib, shape, a, b, ba, bb, ldc=shape.N - 1), RTK_ERR_BAD_ARG)    # ldc < N
    short = Operand(case.A, 1, shape)
    short.ld = shape.K - 1
    untouched(launch(lib, shape, short, b, ba, bb), RTK_ERR_BAD_ARG)                 # ld shorter than the row (K-major)
    short = Operand(case.B, 0, shape)
    short.ld = shape.N - 1
    untouched(launch(lib, shape, a, short, ba, bb), RTK_ERR_BAD_ARG)                 # (M-major)
    untouched(launch(lib, shape, a, b, None, bb), RTK_ERR_BAD_ARG)                   # null bounds
    untouched(launch(lib, shape, a, b, ba, None), RTK_ERR_BAD_ARG)
    rc, h, ldc = launch(lib, shape, a, b, ba, bb)                                    # and the full call is taken
    assert rc == 0 and not differences(read_c(shape, h, ldc), case.model.C, case.valid)


# ---- rtk_absmax_f32 ---------------------------------------------------------------------------------------------------
PAD = np.array([0x7149F2CA, 0x7F800000, 0x7FC00000, 0xFF800000, 0xFFC00001], dtype=np.uint32).view(F32)   # 1e30, inf, nan


class Matrix:
    """rows x cols floats of pitch ld on the device, `off` floats behind a 16-byte boundary, garbage everywhere else"""
    def __init__(self, rows, cols, ld, off=0, fill=None):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        n = off + rows * ld + 8
        self.t = torch.from_numpy(np.resize(PAD, n).copy()).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.view = torch.as_strided(self.t, (rows, cols), (ld, 1), off)
        if fill is None:            # magnitudes below 1, both signs, zeros
            g = torch.Generator(device="cuda").manual_seed(rows * 31 + cols)
            self.view.copy_((torch.rand(rows, cols, device="cuda", generator=g) - 0.5) * 1.75)
            self.view[:, ::7] = 0.0
        else:
            self.view.fill_(fill)
        self.out = torch.empty(1, dtype=torch.float32, device="cuda")

    def absmax(self, lib, rows=None, cols=None):
        self.out.fill_(float("nan") if self.rows % 2 else -7.0)         # garbage before the call
        rc = lib.rtk_absmax_f32(self.t.data_ptr() + 4 * self.off, self.rows if rows is None else rows,
                                self.cols if cols is None else cols, self.ld, self.out.data_ptr(), _stream())
        assert rc == 0, lib.rtk_last_error_string()
        return self.out.cpu().numpy()[0]

    def positions(self):
        """(row, col): first and last element, the last lane of the last full vector (of the folded row when the matrix
        is contiguous), each scalar-tail position, the last column of the first, a middle and the last row, the first
        column of the last row"""
        R, C = self.rows, self.cols
        pos = {(0, 0), (R - 1, C - 1), (0, C - 1), (R // 2, C - 1), (R - 1, 0)}
        total = R * C if self.ld == C else C
        base = 0 if self.ld == C else (R - 1) * C
        for i in [total // 4 * 4 - 1] + list(range(total // 4 * 4, total)):
            if i >= 0:
                pos.add(((base + i) // C, (base + i) % C))
        return sorted(pos)


ABSMAX_SHAPES = [      # rows, cols, ld, off
    (1, 16384, 16384, 0),             # the four-deep vector loop alone
    (1, 16384 + 1028, 16384 + 1028, 0),   # four-deep, then one-deep
    (1, 1000, 1000, 0),               # the one-deep vector loop alone
    (7, 1001, 1001, 0), (3, 1002, 1002, 0), (5, 1003, 1003, 0),      # contiguous, folded: cols % 4 = 1, 2, 3 in the tail
    (1, 3, 3, 0), (1, 1, 1, 0), (2, 2, 2, 0),                         # below one vector
    (3, 5, 8, 0), (5, 1001, 1004, 0), (6, 1003, 1008, 0), (4, 1000, 1012, 0), (3, 16384 + 1030, 16384 + 1032, 0),   # ld > cols, ld % 4 == 0
    (5, 1002, 1003, 0), (3, 17, 19, 0),                               # ld % 4 != 0: scalar loads
    (3, 1000, 1000, 1), (4, 1001, 1004, 1), (1, 16384 + 1028, 16384 + 1028, 3),      # base off its alignment
    (4100, 5, 5, 0), (4100, 5, 8, 0), (4100, 5, 7, 1),                # more rows than the grid's 4096
]


@pytest.mark.parametrize("rows,cols,ld,off", ABSMAX_SHAPES, ids=lambda v: str(v))
def test_absmax_finds_the_maximum_wherever_it_is(lib, rows, cols, ld, off):
    mx = Matrix(rows, cols, ld, off)
    host = mx.view.cpu().numpy().copy()
    assert np.abs(host).max() < 1.0
    assert mx.absmax(lib) == np.abs(host).max()
    for n, (r, c) in enumerate(mx.positions()):
        value = F32((-1.0) ** n * (123.5 + n))
        old = host[r, c]
        host[r, c] = value
        mx.view[r, c] = float(value)
        got = mx.absmax(lib)
        assert got == np.abs(host).max() == abs(value), f"maximum at ({r}, {c}): got {got!r}"
        host[r, c] = old
        mx.view[r, c] = float(old)


def test_absmax_over_the_column_block_clamp(lib):
    """2049 * 16384 + 5 contiguous floats: more column blocks than the grid's 2048, and a scalar tail"""
    n = 2049 * 16384 + 5
    x = torch.rand(n + 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) - 0.5
    x[n:] = 1e30
    out = torch.empty(1, device="cuda")
    assert float(x[:n].abs().max()) <= 0.5
    for k, i in enumerate((0, n - 1, n - 2, n - 5, n - 6, 2048 * 16384 - 1, 2048 * 16384, 2048 * 16384 + 4 * 255 + 3, n // 2 + 1)):
        value = (-1.0) ** k * (2.5 + k)
        old = float(x[i])
        x[i] = value
        out.fill_(float("nan"))
        assert lib.rtk_absmax_f32(x.data_ptr(), 1, n, n, out.data_ptr(), _stream()) == 0
        assert float(out) == abs(value) == float(x[:n].abs().max()), f"maximum at {i}"
        x[i] = old


def test_absmax_values(lib):
    def bits(v):
        return int(np.array([v], dtype=F32).view(np.uint32)[0])

    for rows, cols, ld, off in ((5, 1003, 1008, 0), (3, 1001, 1001, 0), (4, 10, 11, 1)):
        z = Matrix(rows, cols, ld, off, fill=-0.0)
        assert bits(z.absmax(lib)) == 0, "-0.0 only gives +0.0"
        z.view[rows - 1, cols - 1] = -2.0 ** -140
        z.view[0, 0] = 2.0 ** -149
        assert bits(z.absmax(lib)) == bits(2.0 ** -140), "a subnormal maximum"
        z.view[rows // 2, 1] = float("nan")
        z.view[0, cols - 1] = -float("nan")
        z.view[rows - 1, 0] = torch.tensor(np.array([0xFFC00001], dtype=np.uint32).view(F32))[0]
        assert bits(z.absmax(lib)) == bits(2.0 ** -140), "nans of both signs are skipped"
        z.view[rows - 1, cols - 2] = -3.25
        assert z.absmax(lib) == 3.25, "a negative maximum"
        z.view[rows // 2, cols - 1] = -float("inf")
        assert z.absmax(lib) == np.inf, "an inf element gives inf"
        assert bits(z.absmax(lib, rows=0)) == 0 and bits(z.absmax(lib, cols=0)) == 0
        nan = Matrix(rows, cols, ld, off, fill=float("nan"))
        nan.view[::2] = -float("nan")
        assert bits(nan.absmax(lib)) == 0, "an all-nan input gives 0"
