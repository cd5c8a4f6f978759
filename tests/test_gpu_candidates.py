"""Candidate scoring on the MI355X (``ops.score_candidates`` / ``score_triples``, ``rtk_score_candidates_*``):
parity with the golden vectors, the header's float64 bound, bit-for-bit geometry independence, gradients against
float64 autograd, bad ids, empty shapes, and the 1 M-entity bf16 problem."""
import numpy as np
import pytest
import torch

import gen
from oracle import score_oracle as orc

pytestmark = pytest.mark.gpu

Z_TOL, P_TOL = 2e-5, 3e-6


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def dev(*xs):
    return [torch.as_tensor(x).cuda() for x in xs]


def case_inputs(meta_case, shared=False):
    c = meta_case
    core, R, S, O = gen.make_params(c["n_ent"], c["n_rel"], tuple(c["rank"]), c["seed"], shared=shared)
    h, r = gen.make_queries(c["n_ent"], c["n_rel"], c["batch"], c["seed"])
    assert gen.digest(core, R, S, O, h, r) == c["inputs_sha256"]
    return core, R, S, O, h, r


def perms(B, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int64)


def bound(c, bf16):
    """gamma(m + 6) of include/rtucker_hip.h for rank c."""
    w = 8 if bf16 else 4
    m = w * -(-c // (64 * w))
    n = m + 6
    return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


def params(n_ent, n_rel, rank, seed, dtype=torch.float32, shared=False):
    core, R, S, O = dev(*gen.make_params(n_ent, n_rel, rank, seed, shared=shared))
    if shared:
        O = S
    return [t.to(dtype) for t in (core, R, S, O)]


@pytest.mark.parametrize("mode", ["asym", "sym"])
@pytest.mark.parametrize("size", ["tiny", "medium"])
def test_reference_parity(rt, golden, golden_meta, size, mode):
    core, R, S, O, h, r = case_inputs(golden_meta["cases"][f"{size}_{mode}"], shared=(mode == "sym"))
    g = golden(f"{size}_{mode}")
    dcore, dR, dS, dO, dh, dr = dev(core, R, S, O, h, r)
    if mode == "sym":
        dO = dS
    B, N = g["probs"].shape
    cand = perms(B, N, 11)
    dc = torch.from_numpy(cand).cuda()
    z = rt.score_candidates(dcore, dR, dS, dO, dh, dr, dc, sigmoid=False).cpu().numpy()
    pf = rt.score_candidates(dcore, dR, dS, dO, dh, dr, dc, sigmoid_mode="fast").cpu().numpy()
    pe = rt.score_candidates(dcore, dR, dS, dO, dh, dr, dc, sigmoid_mode="exact").cpu().numpy()
    rows = np.arange(B)[:, None]
    zr, pr = g["logits"][rows, cand], g["probs"][rows, cand]
    assert np.max(np.abs(z - zr) / (1 + np.abs(zr))) <= Z_TOL
    assert np.abs(pf - pr).max() <= P_TOL
    assert np.abs(pe - pr).max() <= P_TOL
    if size != "tiny":
        return
    # gradients: (P_cand * w[d, cand]).sum().backward() reproduces the 1-vs-N fixture gradients
    leaves = [t.clone().requires_grad_(True) for t in (dcore, dR, dS)]
    if mode == "sym":
        T = rt.SFTucker(leaves[0], [leaves[1]], 2, leaves[2])
        model = rt.SymmetricR_TuckER((N, R.shape[0]), core.shape)
    else:
        leaves.append(dO.clone().requires_grad_(True))
        T = rt.Tucker(leaves[0], leaves[1:])
        model = rt.AsymmetricR_TuckER((N, R.shape[0]), core.shape)
    P = model.score_candidates(dh, dr, dc)(T)
    w = torch.from_numpy(g["w"][rows, cand]).cuda()
    (P * w).sum().backward()
    for i, leaf in enumerate(leaves):
        np.testing.assert_allclose(leaf.grad.cpu().numpy(), g[f"grad{i}"], rtol=2e-4, atol=2e-5)


def _kernel_case(rt, c, B, K, bf16, ld_mode, seed):
    """v, O, candidate matrix (with duplicates), its (B, K) view for ld_mode 'zero' | 'k' | 'wide'."""
    N = 300
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(seed)
    if c <= 400:
        n_rel = 5
        core, R, S, O = params(N, n_rel, (4, c, c), seed, dtype=dt)
        h = torch.randint(0, N, (B,), device="cuda", generator=g)
        r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
        v = rt.query_vectors(core, R, S, h, r)
    else:
        O = torch.randn((N, c), device="cuda", generator=g).to(dt)
        v = torch.randn((B, c), device="cuda", generator=g)
    base = torch.randint(0, N, (B, K + 5), device="cuda", generator=g)
    base[:, K // 2] = base[:, 0]                                # duplicate ids inside a row
    if ld_mode == "zero":
        cand = base[:1, :K].expand(B, K)
    elif ld_mode == "k":
        cand = base[:, :K].contiguous()
    else:
        cand = base[:, :K]                                      # row stride K + 5
    return v, O, cand


def _raw_scores(rt, v, O, cand, flags):
    lib = rt._lib.load()
    B, K = cand.shape
    ld = cand.stride(0) if B > 1 else K
    out = torch.empty((B, K), dtype=torch.float32, device="cuda")
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    fn = lib.rtk_score_candidates_bf16 if O.dtype == torch.bfloat16 else lib.rtk_score_candidates_f32
    rc = fn(v.data_ptr(), B, v.shape[1], O.data_ptr(), O.shape[0], cand.data_ptr(), ld, K, out.data_ptr(), K, flags,
            ws.data_ptr(), 256, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rtk_last_error_string()
    return out


KERNEL_CASES = [(c, B, K) for c in (1, 3, 5, 200, 256, 400, 1024) for (B, K) in ((1, 1), (5, 7), (512, 64))] + \
               [(200, 4096, 1000), (256, 4096, 1000), (1024, 512, 1000)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("c,B,K", KERNEL_CASES)
def test_kernel_bound(rt, c, B, K, bf16):
    lib = rt._lib
    for ld_mode in ("zero", "k", "wide"):
        v, O, cand = _kernel_case(rt, c, B, K, bf16, ld_mode, seed=c * 7 + K)
        vh = (v.to(torch.bfloat16) if bf16 else v).double().cpu()
        Oc = O.double().cpu()
        cc = cand.cpu()
        rows = Oc[cc]                                           # (B, K, c)
        z64 = torch.einsum("dc,dkc->dk", vh, rows)
        s64 = torch.einsum("dc,dkc->dk", vh.abs(), rows.abs())
        tol = bound(c, bf16) * s64
        z = _raw_scores(rt, v, O, cand, 0).double().cpu()
        assert ((z - z64).abs() <= tol).all(), f"max excess {((z - z64).abs() - tol).max().item():.3e}"
        for flags in (lib.RTK_SCORE_SIGMOID, lib.RTK_SCORE_SIGMOID | lib.RTK_SCORE_SIGMOID_FAST):
            p = _raw_scores(rt, v, O, cand, flags).double().cpu()
            # the logistic's slope is <= 1/4; both forms are within a few ulp of 1
            assert ((p - torch.sigmoid(z64)).abs() <= 0.25 * tol + 4 * 2.0 ** -24).all()


@pytest.mark.parametrize("bf16", [False, True])
def test_geometry_independence(rt, bf16):
    dt = torch.bfloat16 if bf16 else torch.float32
    N, n_rel, B = 4000, 9, 300
    core, R, S, O = params(N, n_rel, (6, 200, 200), 5, dtype=dt)
    g = torch.Generator(device="cuda").manual_seed(5)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    cand = torch.randint(0, N, (B, 97), device="cuda", generator=g)
    full = rt.score_candidates(core, R, S, O, h, r, cand)
    # permuted lists
    perm = torch.randperm(97, device="cuda", generator=g)
    assert torch.equal(rt.score_candidates(core, R, S, O, h, r, cand[:, perm]), full[:, perm])
    # other K, a wider row stride
    assert torch.equal(rt.score_candidates(core, R, S, O, h, r, cand[:, 10:13]), full[:, 10:13])
    wide = torch.cat([cand, cand], 1)
    assert torch.equal(rt.score_candidates(core, R, S, O, h, r, wide[:, :97]), full)
    assert torch.equal(rt.score_candidates(core, R, S, O, h, r, wide), torch.cat([full, full], 1))
    # batch splits
    assert torch.equal(rt.score_candidates(core, R, S, O, h[17:40], r[17:40], cand[17:40]), full[17:40])
    # N: more entity rows behind the same ones
    O2 = torch.cat([O, O[:1000]], 0)
    assert torch.equal(rt.score_candidates(core, R, S, O2, h, r, cand), full)
    # triples are column 0 of a candidate list
    for j in (0, 50):
        assert torch.equal(rt.score_triples(core, R, S, O, h, r, cand[:, j]), full[:, j])
    # a broadcast list: each row equals that row scored alone
    shared = cand[:1].expand(B, 97)
    sb = rt.score_candidates(core, R, S, O, h, r, shared)
    assert torch.equal(rt.score_candidates(core, R, S, O, h[5:6], r[5:6], cand[:1]), sb[5:6])
    # against score_1vN within the 1-vs-N kernel's normwise bound (not bit for bit)
    z = rt.score_candidates(core, R, S, O, h, r, cand, sigmoid=False).double()
    z1 = rt.score_1vN(core, R, S, O, h, r, sigmoid=False).double().gather(1, cand)
    v = rt.query_vectors(core, R, S, h, r)
    vmax = (v.to(dt) if bf16 else v).abs().amax(1, keepdim=True).double()
    omax = O.float().abs().amax(1).double()[cand]
    nb = 2.0 ** -20 * 200 * vmax * omax
    assert ((z - z1).abs() <= nb + 2 * bound(200, bf16) * vmax * omax * 200).all()


def _einsum_scores(core, R, S, O, h, r, cand, sigmoid=True):
    v = torch.einsum("abc,da,db->dc", core, R[r], S[h])
    z = torch.einsum("dc,dkc->dk", v, O[cand])
    return torch.sigmoid(z) if sigmoid else z


def _grad_check(got, ref, what):
    err = (got.double().cpu() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 1e-4 * scale + 1e-7, f"{what}: max |dg| {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("flavour", ["asym", "sym", "doubled"])
def test_gradients_against_float64(rt, flavour):
    N, n_rel, B, K = 700, 6, 64, 33
    rank = (4, 24, 24) if flavour != "doubled" else (8, 48, 48)      # the tangent-space T of training doubles the rank
    shared = flavour == "sym"
    core, R, S, O = params(N, n_rel, rank, 21, shared=shared)
    g = torch.Generator(device="cuda").manual_seed(21)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    cand = torch.randint(0, N, (B, K), device="cuda", generator=g)
    cand[:, 3] = cand[:, 1]
    w = torch.randn((B, K), device="cuda", generator=g)
    leaves = [t.clone().requires_grad_(True) for t in ((core, R, S) if shared else (core, R, S, O))]
    if shared:
        T = rt.SFTucker(leaves[0], [leaves[1]], 2, leaves[2])
        model = rt.SymmetricR_TuckER((N, n_rel), rank)
    else:
        T = rt.Tucker(leaves[0], leaves[1:])
        model = rt.AsymmetricR_TuckER((N, n_rel), rank)
    model.cuda()

    def run():
        for t in leaves:
            t.grad = None
        (model.score_candidates(h, r, cand)(T) * w).sum().backward()
        return [t.grad.clone() for t in leaves]

    g1, g2 = run(), run()
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)                                   # two backward runs: the same bits
    ref = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    O64 = ref[2] if shared else ref[3]
    P = _einsum_scores(ref[0], ref[1], ref[2], O64, h.cpu(), r.cpu(), cand.cpu())
    (P * w.double().cpu()).sum().backward()
    for i, (a, b) in enumerate(zip(g1, ref)):
        _grad_check(a, b.grad, f"{flavour} grad{i}")
    # score_triples' gradient too
    for t in leaves:
        t.grad = None
    model.score_triples(h, r, cand[:, 0])(T).sum().backward()
    ref = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    O64 = ref[2] if shared else ref[3]
    _einsum_scores(ref[0], ref[1], ref[2], O64, h.cpu(), r.cpu(), cand[:, :1].cpu()).sum().backward()
    for i, (a, b) in enumerate(zip(leaves, ref)):
        _grad_check(a.grad, b.grad, f"{flavour} triples grad{i}")


@pytest.mark.parametrize("case", ["skewed", "broadcast"])
def test_gradients_skewed_and_broadcast(rt, case):
    N, n_rel, B, K, c = 5000, 4, 4096, 64, 40
    core, R, S, O = params(N, n_rel, (3, c, c), 8)
    g = torch.Generator(device="cuda").manual_seed(8)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    if case == "skewed":
        cand = torch.randint(0, N, (B, K), device="cuda", generator=g)
        cand[:, 17] = 0                                           # entity 0 in every row: a list of B entries
    else:
        cand = torch.randint(0, N, (1, K), device="cuda", generator=g).expand(B, K)
    w = torch.randn((B, K), device="cuda", generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]

    def run():
        for t in leaves:
            t.grad = None
        (rt.score_candidates(*leaves, h, r, cand, sigmoid=False) * w).sum().backward()
        return [t.grad.clone() for t in leaves]

    g1, g2 = run(), run()
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    ref = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    (_einsum_scores(*ref, h.cpu(), r.cpu(), cand.cpu(), sigmoid=False) * w.double().cpu()).sum().backward()
    for i, (a, b) in enumerate(zip(g1, ref)):
        _grad_check(a, b.grad, f"{case} grad{i}")


def test_out_of_range_ids(rt):
    N, n_rel, B, K = 500, 3, 8, 5
    core, R, S, O = params(N, n_rel, (3, 16, 16), 4)
    h = torch.arange(B, device="cuda")
    r = torch.zeros(B, dtype=torch.int64, device="cuda")
    cand = torch.randint(0, N, (B, K), device="cuda")
    for bad in (N, -1, 10 ** 12):
        c2 = cand.clone()
        c2[3, 2] = bad
        with pytest.raises(IndexError, match="candidate id out of range"):
            rt.score_candidates(core, R, S, O, h, r, c2)
        with rt.index_check("deferred"):
            out = rt.score_candidates(core, R, S, O, h, r, c2)
            assert torch.isnan(out[3, 2])
            ok = torch.ones_like(out, dtype=torch.bool)
            ok[3, 2] = False
            assert torch.isfinite(out[ok]).all()
            assert torch.equal(out[ok], rt.score_candidates(core, R, S, O, h, r, cand)[ok])
            with pytest.raises(IndexError, match="candidate id out of range"):
                rt.check_device_errors()
        rt.check_device_errors()                                   # the word was cleared
    # a bad id adds nothing to the gradients
    c2 = cand.clone()
    c2[3, 2] = N + 4
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
    with rt.index_check("deferred"):
        z = rt.score_candidates(*leaves, h, r, c2, sigmoid=False)
        w = torch.ones_like(z)
        w[3, 2] = 0
        (torch.nan_to_num(z) * w).sum().backward()
        with pytest.raises(IndexError):
            rt.check_device_errors()
    ref = [t.detach().clone().requires_grad_(True) for t in (core, R, S, O)]
    z = rt.score_candidates(*ref, h, r, cand, sigmoid=False)
    w2 = torch.ones_like(z)
    w2[3, 2] = 0
    (z * w2).sum().backward()
    for a, b in zip(leaves, ref):
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-5, atol=1e-6)


def test_empty_shapes(rt):
    core, R, S, O = params(100, 3, (3, 8, 8), 2)
    h = torch.zeros(4, dtype=torch.int64, device="cuda")
    r = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = rt.score_candidates(core, R, S, O, h, r, torch.empty((4, 0), dtype=torch.int64, device="cuda"))
    assert out.shape == (4, 0)
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    assert rt.score_candidates(core, R, S, O, e, e, torch.empty((0, 6), dtype=torch.int64, device="cuda")).shape == (0, 6)
    assert rt.score_triples(core, R, S, O, e, e, e).shape == (0,)
    leaves = [t.clone().requires_grad_(True) for t in (core, R, S, O)]
    rt.score_candidates(*leaves, h, r, torch.empty((4, 0), dtype=torch.int64, device="cuda")).sum().backward()
    assert all(t.grad is not None and not t.grad.any() for t in leaves)


def test_model_eval_uses_tables(rt):
    N, n_rel, rank = 800, 5, (4, 32, 32)
    model = rt.AsymmetricR_TuckER((N, n_rel), rank)
    model.init()
    model.cuda().eval()
    T = rt.Tucker(model.core.data, [model.R.weight.data, model.S.weight.data, model.O.weight.data])
    h = torch.randint(0, N, (50,), device="cuda")
    r = torch.randint(0, n_rel, (50,), device="cuda")
    cand = torch.randint(0, N, (50, 20), device="cuda")
    with torch.no_grad():
        a = model.score_candidates(h, r, cand)(T)
        assert model._tables is not None
        b = rt.score_candidates(model.core, model.R.weight, model.S.weight, model.O.weight, h, r, cand)
        t = model.score_triples(h, r, cand[:, 4])(T)
    assert torch.equal(a, b)
    assert torch.equal(t, a[:, 4])


def test_scale_million_entities_bf16(rt):
    """N = 1 000 000, c 512 bf16, B 8192, K 64: scores and gradients within the bound on a sample, and far less
    memory than the (B, N) matrix (32 GB)."""
    N, n_rel, B, K, c = 1_000_000, 16, 8192, 64, 512
    g = torch.Generator(device="cuda").manual_seed(3)
    bf = torch.bfloat16
    core = (torch.randn((8, c, c), device="cuda", generator=g) * (3.0 / np.sqrt(8 * c * c))).to(bf)
    R = torch.randn((n_rel, 8), device="cuda", generator=g).to(bf)
    S = torch.randn((N, c), device="cuda", generator=g).to(bf)
    O = torch.randn((N, c), device="cuda", generator=g).to(bf)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    cand = torch.randint(0, N, (B, K), device="cuda", generator=g)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    z = rt.score_candidates(core, R, S, O, h, r, cand, sigmoid=False)
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base
    assert fwd_peak < 1 << 30, fwd_peak
    v = rt.query_vectors(core, R, S, h, r)
    rows = torch.arange(0, B, 97, device="cuda")
    vh = v[rows].to(bf).double()
    Os = O[cand[rows]].double()                                   # (s, K, c)
    z64 = torch.einsum("dc,dkc->dk", vh, Os)
    tol = bound(c, True) * torch.einsum("dc,dkc->dk", vh.abs(), Os.abs())
    assert ((z[rows].double() - z64).abs() <= tol).all()
    # gradients: dv and gO through the C entry against float64 on a sample
    lib = rt._lib.load()
    w = torch.randn((B, K), device="cuda", generator=g)
    dv = torch.empty((B, c), dtype=torch.float32, device="cuda")
    gO = torch.empty((N, c), dtype=torch.float32, device="cuda")
    nws = lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rc = lib.rtk_score_candidates_bwd_bf16(w.data_ptr(), K, v.data_ptr(), B, c, O.data_ptr(), N, cand.data_ptr(), K, K,
                                           dv.data_ptr(), gO.data_ptr(), ws.data_ptr(), nws,
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.rtk_last_error_string()
    torch.cuda.synchronize()
    assert nws < 1 << 30, nws
    dv64 = torch.einsum("dk,dkc->dc", w[rows].double(), Os)
    dvt = dv64.abs().amax().item()
    assert (dv[rows].double() - dv64).abs().max().item() <= 1e-5 * dvt
    ents = torch.cat([cand[0, :4], cand[4000, :4]])
    for e in ents.tolist():
        d, k = (cand == e).nonzero(as_tuple=True)
        ref = (w[d, k].double()[:, None] * v[d].double()).sum(0)
        assert (gO[e].double() - ref).abs().max().item() <= 1e-5 * (ref.abs().max().item() + 1e-30) * max(1, len(d))
    untouched = torch.ones(N, dtype=torch.bool, device="cuda")
    untouched[cand.reshape(-1)] = False
    assert not gO[untouched].any()
    # autograd end to end on O alone: finite, and the peak above parameters and the gradient itself stays small
    Og = O.clone().requires_grad_(True)
    del gO, ws
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    (rt.score_candidates(core, R, S, Og, h, r, cand) * w).sum().backward()
    torch.cuda.synchronize()
    grad_bytes = N * c * (4 + 2)                                 # fp32 gradient, then its bf16 copy
    assert torch.cuda.max_memory_allocated() - base - grad_bytes < 1 << 30
    assert torch.isfinite(Og.grad[cand[0]].float()).all()
