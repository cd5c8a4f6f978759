"""GPU tests of the bf16 score kernel (csrc/rtk_score_bf16.hip, rtk_score_packed_bf16) against float64.

The kernel rounds the query vectors to bf16 when they are packed (round to nearest even, as v.bfloat16()), forms
exact products of the bf16 operands on v_mfma_f32_32x32x16_bf16 and sums the KS = ceil(c / 16) k-steps in fp32.
Its error is then that of recursive fp32 summation of 16 KS terms; element-wise, with a factor two of slack,
    logits         |z - z64| <= bound = 2^-23 * 16 KS * sum_k |v^_k| |o_k|,   z64 = v^ . o in float64, v^ = bf16(v)
    probabilities  |p - sigmoid(z64)| <= 3e-6 + bound / 4        (the logistic's slope is <= 1/4)
and the bf16-output form (RTK_SCORE_OUT_BF16) writes the fast probabilities rounded to bf16, bit for bit.  The rows
of v and O carry power-of-two scales over 2^-6 .. 2^6, so a bound of the whole matrix would hide small entries.

The k-step order depends on c alone: at KS > 16 the 4-wave and the 8-wave ("wide") forms, which N and B choose
between, give the same bits, in every logistic mode (test_score_does_not_depend_on_launch_geometry).
Reference path replaced: src/model/asymmetric/R_TuckER.py:47-48 with bf16 parameters.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P_TOL = 3e-6
SENT = -7.0


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _launch(rt, qp, B, c, O, out, N, ld, flags):
    lib = rt._lib.load()
    return lib.rtk_score_packed_bf16(qp.data_ptr(), B, c, O.data_ptr(), N, out.data_ptr() if hasattr(out, "data_ptr") else out,
                                     ld, flags, torch.cuda.current_stream().cuda_stream)


def _score(rt, qp, B, O, flags, pitch, dtype=torch.float32):
    """rtk_score_packed_bf16 into a (B + 1, pitch) buffer filled with a sentinel; checks that nothing was written past
    column N or into the extra row, returns the (B, N) block on the host"""
    N, c = O.shape
    buf = torch.full((B + 1, pitch), SENT, dtype=dtype, device=O.device)
    rt._lib.check(_launch(rt, qp, B, c, O, buf, N, pitch, flags), "rtk_score_packed_bf16")
    torch.cuda.synchronize()
    assert torch.all(buf[B] == SENT), "wrote past row B"
    if pitch > N:
        assert torch.all(buf[:B, N:] == SENT), "wrote past column N"
    return buf[:B, :N].cpu()


def _operands(N, c, B, seed, o_off=0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((B, c), generator=g) * torch.exp2(torch.randint(-6, 7, (B, 1), generator=g).float())
    O = (torch.randn((N, c), generator=g) * torch.exp2(torch.randint(-6, 7, (N, 1), generator=g).float())).bfloat16()
    Od = torch.empty(N * c + o_off, dtype=torch.bfloat16, device="cuda")[o_off:].view(N, c)
    Od.copy_(O)
    return v, O, Od


def _wide(N, c, B):
    """the 8-wave form runs (rtk_score_packed_bf16): KS > 16 and at least 1024 (256-entity, 32-query) tiles"""
    return (c + 15) // 16 > 16 and -(-N // 256) * -(-B // 32) >= 1024


SHAPES = [
    # (N, c, B, pitch, o_off)       what it exercises (KS = ceil(c / 16); "narrow" = 4 waves of 32 entities per workgroup,
    #                               "wide" = 8 waves; blocked = the query sweep is cut into blocks of <= 3 MiB of planes)
    (300, 16, 40, None, 0),         # KS = 1, dense rows, ragged last query tile, N % 32 != 0
    (257, 32, 1, None, 0),          # KS = 2, B = 1, odd N
    (1000, 97, 70, 1001, 0),        # KS = 7, c % 8 != 0: scalar O loads; odd row pitch
    (20, 200, 33, 128, 0),          # KS = 13, N < 32, 128-byte rows: nontemporal stores; one full + one 1-row query tile
    (40003, 200, 64, None, 0),      # KS = 13, 313 x 2 = 626 units over the 512-workgroup grid: several units per workgroup
    (999, 256, 96, 1024, 0),        # KS = 16 (the last two-chain instantiation), nontemporal stores
    (500, 64, 48, None, 1),         # KS = 4, O one element off its 16-byte alignment: scalar loads at c % 8 == 0
    (1500, 272, 100, None, 0),      # KS = 17 narrow
    (1100, 272, 5800, 1152, 0),     # KS = 17 narrow, blocked: 182 query tiles in two blocks of 91
    (600, 288, 64, 601, 1),         # KS = 18 narrow, O misaligned (scalar loads), odd pitch
    (4101, 384, 2000, None, 0),     # KS = 24 wide (17 x 63 tiles), odd N (bf16: the last column stored alone)
    (777, 512, 50, None, 0),        # KS = 32 narrow
    (2600, 512, 3100, 2688, 0),     # KS = 32 wide, blocked: 97 query tiles in two blocks of 49; nontemporal stores
]


@pytest.mark.parametrize("N,c,B,pitch,o_off", SHAPES)
def test_bf16_score_against_float64(rt, N, c, B, pitch, o_off):
    L = rt._lib
    ks = (c + 15) // 16
    pitch = pitch or N
    v, O, Od = _operands(N, c, B, 13 * N + c, o_off)
    vh = v.bfloat16().double().numpy()
    O64 = O.double().numpy()
    z64 = vh @ O64.T
    bound = 2.0 ** -23 * 16 * ks * (np.abs(vh) @ np.abs(O64).T)
    with np.errstate(over="ignore"):
        p64 = 1.0 / (1.0 + np.exp(-z64))
    qp = rt.pack_query_vectors(v.cuda(), torch.bfloat16)
    form = "wide" if _wide(N, c, B) else "narrow"

    z = _score(rt, qp, B, Od, 0, pitch).double().numpy()
    err = np.max(np.abs(z - z64) / bound)
    print(f"N={N} c={c} B={B} ({form}): logits max |dz| / bound = {err:.2e}")
    assert err <= 1.0
    for name, flags in (("exact", L.RTK_SCORE_SIGMOID), ("fast", L.RTK_SCORE_SIGMOID | L.RTK_SCORE_SIGMOID_FAST)):
        p = _score(rt, qp, B, Od, flags, pitch)
        perr = np.max(np.abs(p.double().numpy() - p64) / (P_TOL + bound / 4))
        print(f"  {name} logistic: max |dp| / (3e-6 + bound / 4) = {perr:.2e}")
        assert perr <= 1.0, name
    # bf16 scores: the fast probabilities rounded.  Rows are stored as 4-byte column pairs, so the bf16 pitch is even.
    pb = _score(rt, qp, B, Od, flags | L.RTK_SCORE_OUT_BF16, pitch + (pitch & 1), torch.bfloat16)
    assert torch.equal(pb.view(torch.int16), p.bfloat16().view(torch.int16))
    # run to run
    again = _score(rt, qp, B, Od, 0, pitch).double().numpy()
    assert np.array_equal(again, z)


@pytest.mark.parametrize("c", [272, 512])
def test_score_does_not_depend_on_launch_geometry(rt, c):
    """N = 8192, B = 1024 runs the 8-wave form (32 x 32 tiles); a block of 2048 entities scored alone (8 x 32) and the
    first 64 queries scored alone (32 x 2) run the 4-wave form.  The scores of the overlap are the same bits: entity
    sharding and per-batch relation tables (the bf16 table build is this kernel with K = a) do not change a score."""
    L = rt._lib
    N, B, NB, QB = 8192, 1024, 2048, 64
    assert _wide(N, c, B) and not _wide(NB, c, B) and not _wide(N, c, QB)
    v, _, Od = _operands(N, c, B, c)
    vd = v.cuda()
    qp, qp_sub = rt.pack_query_vectors(vd, torch.bfloat16), rt.pack_query_vectors(vd[:QB], torch.bfloat16)
    fast = L.RTK_SCORE_SIGMOID | L.RTK_SCORE_SIGMOID_FAST
    for name, flags, dt in (("logits", 0, torch.float32), ("exact", L.RTK_SCORE_SIGMOID, torch.float32),
                            ("fast", fast, torch.float32), ("fast bf16", fast | L.RTK_SCORE_OUT_BF16, torch.bfloat16)):
        full = _score(rt, qp, B, Od, flags, N, dt)
        cols = _score(rt, qp, B, Od[:NB], flags, NB, dt)
        rows = _score(rt, qp_sub, QB, Od, flags, N, dt)
        d_cols = int((full[:, :NB] != cols).sum())
        d_rows = int((full[:QB] != rows).sum())
        print(f"c={c} {name}: entries that differ from the 8-wave launch: entity block {d_cols}, query subset {d_rows}")
        assert d_cols == 0, f"{name}: an entity block scored alone differs from the full launch"
        assert d_rows == 0, f"{name}: a query subset scored alone differs from the full launch"


def test_refusals_leave_the_output_untouched(rt):
    """Each documented refusal returns its status before anything is launched.  Every call is also shaped so that a
    launch would stay inside the buffer (B = 1 and N <= the buffer's width)."""
    L = rt._lib
    lib = L.load()
    N, c = 64, 512
    _, _, Od = _operands(N, c, 1, 5)
    qp = rt.pack_query_vectors(torch.ones((1, c), device="cuda"), torch.bfloat16)
    buf = torch.full((2, 2 * N), SENT, dtype=torch.float32, device="cuda")
    fast = L.RTK_SCORE_SIGMOID | L.RTK_SCORE_SIGMOID_FAST
    obf = fast | L.RTK_SCORE_OUT_BF16
    cases = [
        ("c = 513", dict(c=513), -3),
        ("ld_out < N", dict(ld=N - 1), -1),
        ("ld_out >= 2^24", dict(ld=1 << 24), -3),
        ("OUT_BF16 without a logistic", dict(flags=L.RTK_SCORE_OUT_BF16), -3),
        ("OUT_BF16 with the exact logistic", dict(flags=L.RTK_SCORE_SIGMOID | L.RTK_SCORE_OUT_BF16), -3),
        ("misaligned bf16 out", dict(flags=obf, out=buf.data_ptr() + 2), -1),
    ]
    for name, kw, want in cases:
        rc = _launch(rt, qp, 1, kw.get("c", c), Od, kw.get("out", buf), N, kw.get("ld", N), kw.get("flags", 0))
        torch.cuda.synchronize()
        assert rc == want, f"{name}: status {rc}, expected {want}"
        assert torch.all(buf == SENT), f"{name}: the refused call wrote to out"
    assert lib.rtk_score_packed_bf16(None, 1, c, Od.data_ptr(), N, buf.data_ptr(), N, 0, None) == -1
    # and the same buffer takes a valid launch afterwards (the refusals left no sticky state behind)
    rt._lib.check(_launch(rt, qp, 1, c, Od, buf, N, N, fast), "rtk_score_packed_bf16")
    torch.cuda.synchronize()
    assert torch.all(buf[0, N:] == SENT) and torch.all(buf[1] == SENT) and not torch.any(buf[0, :N] == SENT)
