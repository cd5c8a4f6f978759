"""Parity at BASELINE.json's full sizes through size-independent properties (the oracle needs
seconds to minutes at these sizes, so only samples are evaluated exactly):

* shard consistency -- the scores of a row block of O computed on their own are BIT-IDENTICAL to
  the same columns of the full computation (every entity column is scaled, split and accumulated
  independently of the others): this is what makes entity sharding (sharded.py) exact.  One stated
  exception: at the WN18RR shape on one GPU the column-group kernel sums every fifth 32-column group
  as four K-range chains (`ops.cg_fifth_group_columns`); those columns agree with the sharded run
  to the score tolerance, all others bit for bit.  The bf16 score kernel has no exception: its
  4-wave and 8-wave forms, which the entity and query counts choose between, sum the k-steps in one
  order, so a block of entities or of queries scored on its own has the bits of the full launch;
* cross-implementation agreement -- the wave-specialised kernel, the two-workgroup kernel and
  the exact-fp32 MFMA GEMM are three independent implementations of the same product;
* sampled entries against the float64 oracle.
"""

import numpy as np
import pytest
import torch

import gen
from oracle import score_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available()
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def test_c2_wn18rr_full_size_properties(rt, monkeypatch):
    n_ent, n_rel, B, rank = 40943, 22, 512, (10, 200, 200)
    core, R, S, O = gen.make_params(n_ent, n_rel, rank, 322)
    h, r = gen.make_queries(n_ent, n_rel, B, 1234)
    d = [torch.from_numpy(x).cuda() for x in (core, R, S, O)]
    hh, rr = torch.from_numpy(h).cuda(), torch.from_numpy(r).cuda()
    z = rt.score_1vN(*d, hh, rr, sigmoid=False)
    # shard consistency, ragged 8-way split like bench.py --gpus 8
    sh = rt.EntityShards(n_ent, 8)
    from r_tucker_amd.ops import cg_fifth_group_columns
    fifth = torch.from_numpy(cg_fifth_group_columns(n_ent, rank[2])).cuda()
    assert 0.15 < float(fifth.float().mean()) < 0.25          # every fifth group of 32 columns
    for rank_id in (0, 3, 7):
        lo, hi = sh.bounds(rank_id)
        zs = rt.score_1vN(d[0], d[1], d[2], sh.take(d[3], rank_id), hh, rr, sigmoid=False)
        same = ~fifth[lo:hi]
        assert torch.equal(zs[:, : hi - lo][:, same], z[:, lo:hi][:, same])
        dz = (zs[:, : hi - lo] - z[:, lo:hi]).abs() / (1 + z[:, lo:hi].abs())
        assert float(dz.max()) <= 2e-5
    # three implementations
    z_exact = rt.score_1vN(*d, hh, rr, sigmoid=False, exact=True)
    err = ((z - z_exact).abs() / (1 + z_exact.abs())).max().item()
    assert err <= 2e-5, err
    # sampled entries vs float64
    rng = np.random.default_rng(0)
    qs, es = rng.choice(B, 48, replace=False), rng.choice(n_ent, 300, replace=False)
    ze = orc.logits_exact(core, R, S, O[es], h[qs], r[qs])
    zg = z[torch.from_numpy(qs).cuda()][:, torch.from_numpy(es).cuda()].cpu().numpy()
    assert np.max(np.abs(zg - ze) / (1 + np.abs(ze))) <= 2e-5
    # probabilities: monotone in the logits, in (0, 1], row sums match the logits' sigmoid
    p = rt.score_1vN(*d, hh, rr)
    assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0
    assert torch.allclose(p.double().sum(1), torch.sigmoid(z.double()).sum(1), rtol=1e-6)


def test_c2_kernels_agree_v3_vs_ws(rt):
    """Same inputs through the three split-fp16 kernels (rtk_score_1vN_f32 with each kernel hint)."""
    L = rt._lib
    lib = L.load()
    n_ent, n_rel, B, (a, b, c) = 40943, 22, 512, (10, 200, 200)
    core, R, S, O = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, (a, b, c), 322)]
    h, r = [torch.from_numpy(x).cuda() for x in gen.make_queries(n_ent, n_rel, B, 77)]
    ws = torch.zeros(lib.rtk_workspace_bytes(L.RTK_F32, B, n_rel, a, b, c), dtype=torch.uint8, device="cuda")
    outs = []
    for hint in (L.RTK_SCORE_KERNEL_CG, L.RTK_SCORE_KERNEL_WS, L.RTK_SCORE_KERNEL_V3):
        z = torch.empty((B, n_ent), dtype=torch.float32, device="cuda")
        L.check(lib.rtk_score_1vN_f32(core.data_ptr(), a, b, c, R.data_ptr(), n_rel, S.data_ptr(), n_ent, O.data_ptr(),
                                      n_ent, r.data_ptr(), h.data_ptr(), B, z.data_ptr(), n_ent, hint, ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream().cuda_stream), "rtk_score_1vN_f32")
        torch.cuda.synchronize()
        outs.append([float(z.double().sum()), float(z.double().abs().sum()), float(z[17, 4093]), float(z[511, 40942])])
    a = outs[0]
    for b in outs[1:]:
        assert abs(a[0] - b[0]) <= 1e-6 * a[1] and abs(a[2] - b[2]) <= 2e-5 * (1 + abs(a[2])) and abs(a[3] - b[3]) <= 2e-5 * (1 + abs(a[3]))


def test_c5_shard_bf16_full_size_properties(rt):
    """One GPU's share of BASELINE.json configs[4]: 125 000 of 1 M entities, rank (256,512,512),
    batch 8192, bf16 (4.1 GB of fp32 scores)."""
    n_loc, n_rel, B, rank = 125000, 1000, 8192, (256, 512, 512)
    a, b, c = rank
    g = torch.Generator(device="cuda").manual_seed(5)
    core = (torch.randn(rank, generator=g, device="cuda") * (3.0 / np.sqrt(a * b * c))).bfloat16()
    R = torch.randn((n_rel, a), generator=g, device="cuda").bfloat16()
    S = torch.randn((n_loc, b), generator=g, device="cuda").bfloat16()     # subject lookups restricted to the shard's ids
    O = torch.randn((n_loc, c), generator=g, device="cuda").bfloat16()
    h = torch.randint(0, n_loc, (B,), generator=g, device="cuda")
    r = torch.randint(0, n_rel, (B,), generator=g, device="cuda")
    z = rt.score_1vN(core, R, S, O, h, r, sigmoid=False)
    assert z.shape == (B, n_loc) and bool(torch.isfinite(z).all())
    # shard consistency (bit-exact): a 3000-row sub-block
    zs = rt.score_1vN(core, R, S, O[50000:53000].contiguous(), h, r, sigmoid=False)
    assert torch.equal(zs, z[:, 50000:53000])
    # probabilities written as bf16 by the 8-wave kernel = the fp32 probabilities rounded
    del zs
    p32 = rt.score_1vN(core, R, S, O, h, r)
    pb = rt.score_1vN(core, R, S, O, h, r, out_dtype=torch.bfloat16)
    assert pb.dtype == torch.bfloat16 and pb.shape == p32.shape
    for lo in range(0, B, 1024):                       # in slices: the comparison needs a rounded copy
        assert torch.equal(pb[lo:lo + 1024], p32[lo:lo + 1024].to(torch.bfloat16))
    del p32, pb
    # a query subset scored alone runs the 4-wave form (489 x 2 tiles): the same bits as the 8-wave launch
    v = rt.query_vectors(core, R, S, h, r)
    zq = torch.empty((64, n_loc), dtype=torch.float32, device="cuda")
    rt.score_packed_into(rt.pack_query_vectors(v[:64], torch.bfloat16), 64, O, zq, sigmoid=False)
    assert torch.equal(zq, z[:64])
    del zq
    # sampled rows in full against float64, element-wise: the score kernel against the bf16-rounded stage-1 vectors
    # (|dz| <= 2^-23 * 16 * 32 * sum_k |v^_k| |o_k|, tests/test_gpu_score_bf16.py), stage 1 against the oracle
    # (|dv| <= (a + b + 2) * 2^-23 * v_abs, tests/test_gpu_stage1_bounds.py)
    qs = torch.tensor([0, 1, 31, 32, 4095, 4096, 8190, 8191], device="cuda")
    O64 = O.double().cpu().numpy()
    vh = v[qs].bfloat16().double().cpu().numpy()
    zg = z[qs].double().cpu().numpy()
    bound = 2.0 ** -23 * 16 * ((c + 15) // 16) * (np.abs(vh) @ np.abs(O64).T)
    err = np.max(np.abs(zg - vh @ O64.T) / bound)
    G64, R64, S64 = [x.double().cpu().numpy() for x in (core, R, S)]
    hq, rq = h[qs].cpu().numpy(), r[qs].cpu().numpy()
    v64 = orc.query_vectors_exact(G64, R64, S64, hq, rq)
    v_abs = orc.query_vectors_exact(np.abs(G64), np.abs(R64), np.abs(S64), hq, rq)
    verr = np.max(np.abs(v[qs].double().cpu().numpy() - v64) / ((a + b + 2) * 2.0 ** -23 * v_abs))
    print(f"C5 shard: scores max |dz| / bound = {err:.2e}, stage 1 max |dv| / bound = {verr:.2e}")
    assert err <= 1.0 and verr <= 1.0
    del z
    torch.cuda.empty_cache()
