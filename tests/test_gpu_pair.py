"""GPU tests of rtk_pair_vectors_* (csrc/rtk_pair.hip): the pair vectors u of (h, ?, t) queries.

u against the float64 model within tau_u (tests/relation_model.py, which states the bound from the bounds the score
kernels are tested to), through the ctypes ABI so that b != c is reachable, on the smallest shapes at which each
mechanism of the kernel can go wrong; and the bits of a row of u: they depend on the query alone, not on the batch,
the query's place in it or the grid."""
import numpy as np
import pytest
import torch

import relation_model as rm

pytestmark = pytest.mark.gpu

N_ENT = 50


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _operands(a, b, c, B, seed, bf16):
    """core slabs and rows of S and O with power-of-two scales over 2^-6 .. 2^6; float32 arrays holding the values the
    device gets (bf16: rounded)."""
    core = rm.scaled((a, b * c), seed).reshape(a, b, c)
    S, O = rm.scaled((N_ENT, b), seed + 1), rm.scaled((N_ENT, c), seed + 2)
    rng = np.random.default_rng(seed + 3)
    h, t = rng.integers(0, N_ENT, B), rng.integers(0, N_ENT, B)
    if bf16:
        core, S, O = rm.bf16_round(core), rm.bf16_round(S), rm.bf16_round(O)
    return core, S, O, h.astype(np.int64), t.astype(np.int64)


def _dev(x, bf16):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.bfloat16() if bf16 else t


def _pair_abi(rt, core, S, O, h, t, bf16, pad=3):
    """rtk_pair_vectors_* on device operands -> u (B, a) on the host.  u has a pitch of a + pad and the workspace a
    tail behind the queried size, both filled with a sentinel that must survive; the error word must stay 0."""
    lib = rt._lib.load()
    a, b, c = core.shape
    B = h.numel()
    need = lib.rtk_pair_vectors_workspace_bytes(1 if bf16 else 0, B, a, b, c)
    assert need > 0
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    ws[:256].zero_()
    u = torch.full((B, a + pad), -7.0, dtype=torch.float32, device="cuda")
    fn = lib.rtk_pair_vectors_bf16 if bf16 else lib.rtk_pair_vectors_f32
    rt._lib.check(fn(core.data_ptr(), a, b, c, S.data_ptr(), S.shape[0], O.data_ptr(), O.shape[0], h.data_ptr(), t.data_ptr(),
                     B, u.data_ptr(), a + pad, None, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream),
                  "rtk_pair_vectors")
    torch.cuda.synchronize()
    assert torch.all(ws[need:] == 0x5A), "wrote past the workspace"
    assert torch.all(u[:, a:] == -7.0), "wrote past a row of u"
    assert int(ws[:4].view(torch.int32).item()) == 0
    return u[:, :a].cpu().numpy()


BOTH = [
    (1, 1, 4, 1),            # smallest shape
    (3, 5, 4, 33),           # b < 32
    (10, 36, 36, 70),        # b % 32 != 0, KS 3
    (10, 200, 200, 70),      # the WN18RR rank
    (2, 160, 64, 5),         # more than one tile per slab
    (7, 32, 16, 300),        # few tiles, many query tiles: qsplit > 1
    (1040, 64, 4, 33),       # more than 512 tiles: a workgroup takes several
]
F32_ONLY = [(2, 208, 208, 40)]                                           # KS 13
BF16_ONLY = [
    (3, 20, 100, 33),        # c % 8 != 0, scalar loads
    (2, 40, 512, 40),        # KS 32
    (1040, 64, 8, 33),       # more than 512 tiles
]
CASES = [(s, False) for s in BOTH + F32_ONLY] + [(s, True) for s in BOTH + BF16_ONLY]


@pytest.mark.parametrize("shape,bf16", CASES, ids=[f"{'bf16' if f else 'f32'}-{'x'.join(map(str, s))}" for s, f in CASES])
def test_u_against_float64(rt, shape, bf16):
    a, b, c, B = shape
    core, S, O, h, t = _operands(a, b, c, B, 11 * a + 3 * b + c, bf16)
    u64, tau_u = rm.u_bounds(core, S, O, h, t, bf16)
    u = _pair_abi(rt, _dev(core, bf16), _dev(S, bf16), _dev(O, bf16), torch.from_numpy(h).cuda(), torch.from_numpy(t).cuda(),
                  bf16)
    assert np.all(np.isfinite(u))
    excess = np.abs(u - u64) - tau_u
    ratio = np.max(np.abs(u - u64) / np.maximum(tau_u, 1e-300))
    rel = np.median(tau_u / np.maximum(np.abs(u64), 1e-300))
    print(f"a={a} b={b} c={c} B={B} {'bf16' if bf16 else 'f32'}: max |du| / tau_u = {ratio:.2e} (median tau_u / |u| = {rel:.1e})")
    assert np.all(excess <= 0), f"max |du| / tau_u = {ratio:.3e}"


def _plane_rows(qp, B, K, bf16):
    """The packed planes as (tiles, header 32 floats) and (tiles, planes, ksteps, 2, 32, 8) int16; the rows of the last
    tile past the batch are unwritten, so both come with the mask of the written rows."""
    ks, planes = -(-K // 16), 1 if bf16 else 2
    tile = 128 + planes * ks * 1024
    n_mt = -(-B // 32)
    raw = qp.cpu().numpy()[:n_mt * tile].reshape(n_mt, tile)
    hdr = raw[:, :128].copy().view(np.float32)
    body = raw[:, 128:].copy().view(np.int16).reshape(n_mt, planes, ks, 2, 32, 8)
    live = (np.arange(n_mt * 32) < B).reshape(n_mt, 32)
    return hdr[live], body.transpose(0, 4, 1, 2, 3, 5)[live]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("rank,B", [((10, 36, 36), 70), ((7, 32, 32), 300)])
def test_rows_do_not_depend_on_the_batch(rt, rank, B, bf16):
    """bit for bit: the same queries permuted, the first 33 alone (another grid: fewer query tiles, another qsplit),
    three queries each alone, a second run; and packed=True gives the planes pack_query_vectors(u) gives."""
    a, b, c = rank
    core, S, O, h, t = _operands(a, b, c, B, 5 + a, bf16)
    G, Sd, Od = _dev(core, bf16), _dev(S, bf16), _dev(O, bf16)
    hd, td = torch.from_numpy(h).cuda(), torch.from_numpy(t).cuda()
    u, qp = rt.pair_vectors(G, Sd, Od, hd, td, packed=True)
    assert u.shape == (B, a) and u.dtype == torch.float32
    again = rt.pair_vectors(G, Sd, Od, hd, td)
    assert torch.equal(u, again)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(B)).cuda()
    assert torch.equal(rt.pair_vectors(G, Sd, Od, hd[perm], td[perm]), u[perm])
    assert torch.equal(rt.pair_vectors(G, Sd, Od, hd[:33], td[:33]), u[:33])
    for d in (0, 31, B - 1):
        assert torch.equal(rt.pair_vectors(G, Sd, Od, hd[d:d + 1], td[d:d + 1]), u[d:d + 1])
    # symmetric model: S is O
    us = rt.pair_vectors(G, Sd, Sd, hd, td)
    us64, tau = rm.u_bounds(core, S, S, h, t, bf16)
    assert np.all(np.abs(us.cpu().numpy() - us64) <= tau)
    want = rt.pack_query_vectors(u, torch.bfloat16 if bf16 else torch.float32)
    torch.cuda.synchronize()
    for x, y in zip(_plane_rows(qp, B, a, bf16), _plane_rows(want, B, a, bf16)):
        assert np.array_equal(x, y)
    assert rt.pair_vectors(G, Sd, Od, hd[:0], td[:0]).shape == (0, a)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_out_of_range_ids(rt, bf16):
    """An id outside its table raises IndexError under "strict" and at check_device_errors() under "deferred"; the id is
    clamped and the other rows of the batch keep their bits."""
    a, b, c, B = 5, 36, 36, 40
    core, S, O, h, t = _operands(a, b, c, B, 77, bf16)
    G, Sd, Od = _dev(core, bf16), _dev(S, bf16), _dev(O, bf16)
    hd, td = torch.from_numpy(h).cuda(), torch.from_numpy(t).cuda()
    good = rt.pair_vectors(G, Sd, Od, hd, td)
    for which, bad, word in (("subject", N_ENT, "subject_idx"), ("subject", -1, "subject_idx"),
                             ("object", N_ENT + 7, "object_idx"), ("object", -2, "object_idx")):
        h2, t2 = hd.clone(), td.clone()
        (h2 if which == "subject" else t2)[17] = bad
        with rt.index_check("strict"):
            with pytest.raises(IndexError, match=word):
                rt.pair_vectors(G, Sd, Od, h2, t2)
        with rt.index_check("deferred"):
            u = rt.pair_vectors(G, Sd, Od, h2, t2)
            keep = torch.arange(B, device="cuda") != 17
            assert torch.equal(u[keep], good[keep]) and torch.isfinite(u[17]).all()
            with pytest.raises(IndexError, match=word):
                rt.check_device_errors()
        rt.check_device_errors()                                        # the word was cleared
