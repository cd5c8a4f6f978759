"""GPU tests of the three split-fp16 score kernels (rtk_score_packed_f32: cg, ws, v3) against the numpy split model of
tests/golden/split_cases.py.

The split x = hi + lo is deterministic arithmetic that numpy reproduces exactly, and the MFMA forms exact products of
fp16 values, so on operands for which no fp32 partial sum can round (max T / g <= 2^23, asserted by the generator) a
kernel must return
    z_model[d, j] = (vh.oh + vh.ol + vl.oh) 2^-(sh_v[d] + sh_o[j])
bit for bit, whatever its summation order -- on every exact family, every shape and every kernel that covers it.
The probabilities are compared with sigmoid(z_model) in float64 under relative bounds derived from the per-step accuracies
(split_cases.p_bound), a real-valued layer under gamma(48 KS) T, and a NaN or an inf in one operand row must stay in its
row / column of the scores.
Reference path replaced: src/model/asymmetric/R_TuckER.py:47-48.
"""
import functools

import numpy as np
import pytest
import torch

import split_cases as sc

pytestmark = pytest.mark.gpu

SENT = -7.0
F32, F64, I32 = np.float32, np.float64, np.int32


# the case of consecutive tests on one shape and family is built once (cases are read-only; the largest holds 100 MB)
_case = functools.lru_cache(maxsize=1)(sc.make_case)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


@pytest.fixture(autouse=True)
def _nothing_is_launched_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the session ends here: {e}", returncode=3)


def _hints(rt, shape):
    """(name, hint) of every kernel that covers the shape, and no hint"""
    L = rt._lib
    table = {"cg": L.RTK_SCORE_KERNEL_CG, "ws": L.RTK_SCORE_KERNEL_WS, "v3": L.RTK_SCORE_KERNEL_V3}
    return [(k, table[k]) for k in shape.kernels] + [("auto", 0)]


class Device:
    """a case's operands on the device: O inside its guarded buffer (o_off floats off a 16-byte boundary), the packed
    query planes of v"""

    def __init__(self, rt, case, v=None, obuf=None):
        s = case.shape
        self.rt, self.shape = rt, s
        self.obuf = torch.from_numpy(case.obuf if obuf is None else obuf).cuda()
        self.O = self.obuf[s.o_off:s.o_off + s.N * s.c].view(s.N, s.c)
        assert (self.O.data_ptr() % 16 == 0) == (s.o_off == 0)
        self.qp = rt.pack_query_vectors(torch.from_numpy(case.v if v is None else v).cuda(), torch.float32)

    def score(self, flags):
        """rtk_score_packed_f32 into a sentinel-filled (B + 1, pitch) buffer -> the (B, N) block on the host; the row past
        B and the columns past N must keep the sentinel"""
        s, rt = self.shape, self.rt
        lib = rt._lib.load()
        buf = torch.full((s.B + 1, s.ld), SENT, dtype=torch.float32, device="cuda")
        rt._lib.check(lib.rtk_score_packed_f32(self.qp.data_ptr(), s.B, s.c, self.O.data_ptr(), s.N, buf.data_ptr(), s.ld, flags,
                                               torch.cuda.current_stream().cuda_stream), "rtk_score_packed_f32")
        torch.cuda.synchronize()
        assert torch.all(buf[s.B] == SENT), "wrote past row B"
        if s.ld > s.N:
            assert torch.all(buf[:s.B, s.N:] == SENT), "wrote past column N"
        return buf[:s.B, :s.N].cpu().numpy()


def _ran(rt, shape, name, hint):
    """on a shape with hints: the hinted kernel is the one that runs"""
    if name != "auto" and shape.o_off == 0:
        assert rt._lib.load().rtk_score_kernel_f32(shape.N, shape.c, hint) == hint, name


def _differs(z, ref32):
    """entries whose bits differ (int32 views), -0.0 and +0.0 taken as equal"""
    return (z.view(I32) != ref32.view(I32)) & ~((z == 0) & (ref32 == 0))


def _report(name, z, ref32, bad):
    dd, jj = np.nonzero(bad)
    with np.errstate(all="ignore"):
        ulps = np.abs(z.view(I32).astype(np.int64) - ref32.view(I32).astype(np.int64))[bad]
    head = ", ".join(f"({d},{j}): {z[d, j]!r} != {ref32[d, j]!r}" for d, j in list(zip(dd, jj))[:6])
    return (f"{name}: {int(bad.sum())} of {bad.size} entries differ from z_model; rows {np.unique(dd)[:12].tolist()} "
            f"columns {np.unique(jj)[:12].tolist()} (of {np.unique(jj).size}); bit distance min {ulps.min()} max {ulps.max()}; {head}")


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_logits_equal_the_model_bit_for_bit(rt, shape, family):
    case = _case(shape, family)                 # asserts max T / g <= 2^23
    ref32 = case.model.z.astype(F32)
    ok = case.valid if case.valid is not None else np.ones(ref32.shape, dtype=bool)
    assert np.array_equal(ref32.astype(F64)[ok], case.model.z[ok])
    dev = Device(rt, case)
    out, failures = {}, []
    for name, hint in _hints(rt, shape):
        _ran(rt, shape, name, hint)
        out[name] = dev.score(hint)
        bad = _differs(out[name], ref32) & ok
        if bad.any():
            failures.append(_report(f"{case.name} {name}", out[name], ref32, bad))
    assert not failures, "\n".join(failures)
    first = out[shape.kernels[0]]
    for name in out:                            # ... and so to each other
        assert not (_differs(out[name], first) & ok).any(), name


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_probabilities_against_the_float64_logistic(rt, shape):
    """both logistic modes on the fewbit case (|z| from 2^-6 to past both saturations) against sigmoid(z_model)"""
    L = rt._lib
    case = _case(shape, "fewbit")
    z = case.model.z
    p64 = sc.sigmoid64(z)
    with np.errstate(under="ignore"):
        p64_32 = p64.astype(F32)
    dev = Device(rt, case)
    failures = []
    for name, hint in _hints(rt, shape):
        for mode, flags, fast in (("exact", L.RTK_SCORE_SIGMOID, False), ("fast", L.RTK_SCORE_SIGMOID | L.RTK_SCORE_SIGMOID_FAST, True)):
            p = dev.score(flags | hint)
            ratio = np.abs(p.astype(F64) - p64) / sc.p_bound(z, fast)
            d, j = np.unravel_index(np.argmax(ratio), ratio.shape)
            print(f"{case.name} {name} {mode}: worst |dp| / bound = {ratio.max():.3f} at z = {z[d, j]:.4f}")
            if not ratio.max() <= 1.0:
                failures.append(f"{name} {mode}: |dp| / bound = {ratio.max():.3f} at z = {z[d, j]!r}: p = {p[d, j]!r}, float64 {p64[d, j]!r}")
            # saturated where the float64 value rounds to 1.0f or 0.0f
            for v in (1.0, 0.0):
                sat = p64_32 == F32(v)
                if not np.array_equal(p[sat], p64_32[sat]):
                    k = np.flatnonzero(p[sat] != v)[0]
                    failures.append(f"{name} {mode}: not exactly {v} at z = {z[sat][k]!r}: {p[sat][k]!r}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["rows", "range"])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.SHAPE_IDS)
def test_real_layer_within_the_chain_bound(rt, shape, kind):
    """|z - z_model| <= gamma(48 KS) T (48 KS + 3 on a fifth group's columns): the rounding of one fp32 chain of 3 * 16 * KS
    terms, and nothing else -- the split itself is in the model"""
    case = sc.real_case(shape, kind)
    m = sc.score_model(case.v, case.O)
    dev = Device(rt, case)
    failures = []
    for name, hint in _hints(rt, shape):
        fifth = None
        if name in ("cg", "auto") and shape.o_off == 0 and "cg" in shape.kernels:
            fifth = rt.ops.cg_fifth_group_columns(shape.N, shape.c, hint)
        z = dev.score(hint).astype(F64)
        ratio = np.abs(z - m.z) / np.maximum(sc.z_bound(m, shape.c, fifth), 2.0 ** -149)
        print(f"{case.name} {name}: worst |z - z_model| / bound = {ratio.max():.4f}" + (f" ({int(fifth.sum())} fifth-group columns)" if fifth is not None and fifth.any() else ""))
        if not ratio.max() <= 1.0:
            d, j = np.unravel_index(np.argmax(ratio), ratio.shape)
            failures.append(f"{name}: |z - z_model| / bound = {ratio.max():.3f} at ({d}, {j}): {z[d, j]!r} against {m.z[d, j]!r}")
    assert not failures, "\n".join(failures)


ISOLATION = sc.SHAPES[1]        # N = 40 943, c = 200, B = 50: cg sets of five, the last group ragged AND a fifth group


@pytest.mark.parametrize("kernel", ["cg", "ws", "v3", "auto"])
def test_a_nan_or_inf_stays_in_its_row_and_column(rt, kernel):
    shape = ISOLATION
    name, hint = [h for h in _hints(rt, shape) if h[0] == kernel][0]
    case = _case(shape, "fewbit")
    fifth = rt.ops.cg_fifth_group_columns(shape.N, shape.c, rt._lib.RTK_SCORE_KERNEL_CG)
    j5 = int(np.flatnonzero(fifth)[3])
    assert fifth[shape.N - 1] and shape.N % 32 != 0 and not fifth[40]
    clean = Device(rt, case).score(hint)
    assert np.isfinite(clean).all()
    # (query row, entity row, element): a fifth-group column, the last column of the ragged last group, a plain one
    for d0, j0, k0 in ((3, j5, 5), (shape.B - 1, shape.N - 1, shape.c - 1), (32, 40, 0)):
        for val in (np.nan, np.inf):
            v, obuf = case.v.copy(), case.obuf.copy()
            v[d0, k0] = val
            obuf[shape.o_off + j0 * shape.c + (k0 + 7) % shape.c] = val
            z = Device(rt, case, v, obuf).score(hint)
            inside = np.zeros(z.shape, dtype=bool)
            inside[d0, :] = True
            inside[:, j0] = True
            assert not np.isfinite(z[inside]).any(), f"{name}: a finite score in row {d0} / column {j0} with {val} planted"
            assert np.array_equal(z.view(I32)[~inside], clean.view(I32)[~inside]), \
                f"{name}: {val} in row {d0} / column {j0} changed {int((z.view(I32) != clean.view(I32))[~inside].sum())} other scores"


@pytest.mark.parametrize("kernel", ["cg", "ws", "v3"])
def test_second_launch_gives_the_same_bits(rt, kernel):
    L = rt._lib
    shape = sc.SHAPES[3]        # N = 36 000, c = 64: cg sets of four and five side by side
    hint = {"cg": L.RTK_SCORE_KERNEL_CG, "ws": L.RTK_SCORE_KERNEL_WS, "v3": L.RTK_SCORE_KERNEL_V3}[kernel]
    dev = Device(rt, sc.real_case(shape, "rows"))
    for flags in (0, L.RTK_SCORE_SIGMOID, L.RTK_SCORE_SIGMOID | L.RTK_SCORE_SIGMOID_FAST):
        a, b = dev.score(flags | hint), dev.score(flags | hint)
        assert np.array_equal(a.view(I32), b.view(I32)), (kernel, flags)
