"""The two routes of the stage-1 backward at the Python level (ops.stage1_backward_route, ops._STAGE1_BWD_GEMM_BYTES):
"gemm" = rtk_query_vectors_bwd_f32 with its two (B, a*b) matrices, "stream" = rtk_query_vectors_bwd_stream_* without.

One small case (N 3003, B 70, rank (5, 64, 64)) through the three callers of the stage-1 backward -- the block loss,
score_1vN(...).sum().backward() and score_candidates -- with the limit patched to 0 (stream) and to 2^62 (gemm): the
loss and the scores are equal, g_S and g_O are equal, g_core is equal where the GEMM form does not split K, and g_R
lies within the sum of the two routes' gamma bounds (the order over j differs).  With bf16 leaves every gradient is
bf16 and within one bf16 ulp of the max-norm of the gemm route's.  Then peak memory at rank (128, 64, 64), B 2048:
with the stream route forward + backward stay below half of ONE of the GEMM form's two matrices.
"""
import numpy as np
import pytest
import torch

import exact_cases as ec
from r_tucker_amd.synthetic import make_params

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -7           # one ulp of a bf16 value g is at most 2^-7 |g|
N_ENT, N_REL, B, RANK, EPS = 3003, 7, 70, (5, 64, 64), 0.1
STREAM, GEMM = 0, 1 << 62


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available()
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


class _Pairs:
    """The attributes DeviceFilter reads from a KG_dataset, for a synthetic (pair -> objects) table."""
    def __init__(self, pairs, lists, n_ent, eps):
        self._pair_slot = {p: i for i, p in enumerate(pairs)}
        self._ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        self._obj = np.asarray([x for l in lists for x in l], dtype=np.int64)
        self.features = np.asarray(pairs, dtype=np.int64)
        self.n_ent, self.label_smoothing = n_ent, eps


def _case(rt, n_ent, rank, batch, seed, dtype, n_subj=None):
    """Parameters (the core scaled by 0.4: nothing saturates), a filter with one empty list, a batch of items; subjects
    repeat, so the row scatter has lists to add."""
    core, R, S, O = make_params(n_ent, N_REL, rank, seed)
    n_subj = n_subj or n_ent
    rng = np.random.default_rng(seed)
    n_pairs = max(batch, 1)
    subj = rng.integers(0, max(2, n_pairs // 2), n_pairs) * (n_subj // max(2, n_pairs // 2) - 1)
    pairs = list(dict.fromkeys((int(s), int(r_)) for s, r_ in zip(subj, rng.integers(0, N_REL, n_pairs))))
    lists = [np.unique(rng.integers(0, n_ent, int(rng.integers(1, 9)))).tolist() for _ in pairs]
    lists[0] = []
    ds = _Pairs(pairs, lists, n_ent, EPS)
    flt = rt.DeviceFilter(ds, "cuda")
    ids = rng.integers(0, len(pairs), batch).astype(np.int64)
    params = [torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype) for x in (core * 0.4, R, S[:n_subj], O)]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    return params, flt, h, r, torch.from_numpy(ids).cuda()


def _run(rt, monkeypatch, limit, fn, params, weight=3.0):
    """value, the leaves' gradients and what the stage-1 backward was called with, under the patched limit."""
    monkeypatch.setattr(rt.ops, "_STAGE1_BWD_GEMM_BYTES", limit)
    seen = []
    inner = rt.ops._stage1_backward

    def spy(core, R, S, h, r, dv, needs):
        seen.append((core, R, S, h, r, dv.clone(), rt.ops.stage1_backward_route(dv.shape[0], *core.shape)))
        return inner(core, R, S, h, r, dv, needs)
    monkeypatch.setattr(rt.ops, "_stage1_backward", spy)
    ps = [p.clone().requires_grad_(True) for p in params]
    out = fn(ps)
    (out.sum() * weight).backward()
    monkeypatch.setattr(rt.ops, "_stage1_backward", inner)
    assert len(seen) == 1
    return out.detach(), [p.grad for p in ps], seen[0]


def _g_r_bound(call):
    """The sum of the two routes' gamma bounds on g_R, from the operands the stage-1 backward received."""
    core, R, S, h, r, dv, _ = call
    ops = [x.detach().float().cpu().numpy() for x in (core, R, S, dv)] + [r.cpu().numpy(), h.cpu().numpy()]
    a, b, c = ops[0].shape
    case = ec.BwdCase("route", dv.shape[0], a, b, c, ops[1].shape[0], ops[2].shape[0])
    return 2.0 * ec.bwd_bounds(case, *ops, 1)[1]


def _compare_fp32(rt, stream, gemm):
    (out_s, g_s, call_s), (out_g, g_g, call_g) = stream, gemm
    assert call_s[6] == "stream" and call_g[6] == "gemm"
    assert torch.equal(out_s, out_g)                                   # the forward does not depend on the route
    assert torch.equal(call_s[5], call_g[5])                           # nor does dv
    a, b, c = call_s[0].shape
    for name, k in (("g_S", 2), ("g_O", 3)):
        assert g_s[k].dtype == torch.float32 and bool((g_s[k] == g_g[k]).all()), name
    assert ec.gcore_splits(B, a, b, c) == 1
    assert bool((g_s[0] == g_g[0]).all()), "g_core"
    err = (g_s[1].double() - g_g[1].double()).abs().cpu().numpy()
    bound = _g_r_bound(call_s)
    print(f"\n[stage-1 route] g_R: largest difference / (2 x gamma bound) {float(np.max(err / np.maximum(bound, 1e-300))):.4f}")
    assert np.all(err <= bound) and g_g[1].abs().max().item() > 0


def _loss(rt, flt, h, r, idc):
    return lambda ps: rt.bce_loss_block_1vN(*ps, 0, N_ENT, h, r, flt, idc, label_smoothing=EPS)


def test_block_loss_fp32_both_routes(rt, monkeypatch):
    params, flt, h, r, idc = _case(rt, N_ENT, RANK, B, 51, torch.float32)
    fn = _loss(rt, flt, h, r, idc)
    _compare_fp32(rt, _run(rt, monkeypatch, STREAM, fn, params), _run(rt, monkeypatch, GEMM, fn, params))


def test_score_1vN_fp32_both_routes(rt, monkeypatch):
    params, _, h, r, _ = _case(rt, N_ENT, RANK, B, 52, torch.float32)
    fn = lambda ps: rt.score_1vN(*ps, h, r)                        # noqa: E731
    _compare_fp32(rt, _run(rt, monkeypatch, STREAM, fn, params), _run(rt, monkeypatch, GEMM, fn, params))


def test_score_candidates_fp32_both_routes(rt, monkeypatch):
    params, _, h, r, _ = _case(rt, N_ENT, RANK, B, 53, torch.float32)
    cand = torch.randint(0, N_ENT, (B, 9), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    fn = lambda ps: rt.score_candidates(*ps, h, r, cand)           # noqa: E731
    _compare_fp32(rt, _run(rt, monkeypatch, STREAM, fn, params), _run(rt, monkeypatch, GEMM, fn, params))


@pytest.mark.parametrize("caller", ["block_loss", "score_1vN", "score_candidates"])
def test_bf16_leaves_both_routes(rt, monkeypatch, caller):
    """Every gradient is bf16; the routes differ by at most 2^-7 max|g| of the gemm route's.  The stream route receives
    the bf16 operands themselves (no fp32 copy), the gemm route upcasts them inside."""
    params, flt, h, r, idc = _case(rt, N_ENT, RANK, B, 54, torch.bfloat16)
    cand = torch.randint(0, N_ENT, (B, 9), device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    fn = {"block_loss": _loss(rt, flt, h, r, idc), "score_1vN": lambda ps: rt.score_1vN(*ps, h, r),
          "score_candidates": lambda ps: rt.score_candidates(*ps, h, r, cand)}[caller]
    out_s, g_s, call_s = _run(rt, monkeypatch, STREAM, fn, params)
    out_g, g_g, call_g = _run(rt, monkeypatch, GEMM, fn, params)
    assert call_s[6] == "stream" and call_g[6] == "gemm" and torch.equal(out_s, out_g)
    assert all(t.dtype == torch.bfloat16 for t in call_s[:3]) and call_s[5].dtype == torch.float32
    for name, x, y in zip(("core", "R", "S", "O"), g_s, g_g):
        assert x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and x.shape == y.shape, name
        top = y.float().abs().max().item()
        assert top > 0 and (x.float() - y.float()).abs().max().item() <= BF16_ULP * top, name


def test_peak_memory_of_the_stream_route(rt, monkeypatch):
    """Rank (128, 64, 64), B 2048, N 3003, fp32, the limit at 16 MiB: a b = 8192, so the GEMM form would take 2 x 67 MB.
    First the sum of what the design holds is shown to stay below B a b 4 / 2, then forward + backward are held to it.
    (The forward demands b == c, and the loss workspace grows with c: the wide mode is the relation's here.)  With the
    default limit the same call takes the gemm route."""
    n_ent, batch, rank, n_subj = 3003, 2048, (128, 64, 64), 3003
    a, b, c = rank
    lib = rt._lib.load()
    assert rt.ops.stage1_backward_route(batch, a, b, c) == "gemm"
    assert lib.rtk_query_bwd_workspace_bytes(batch, a, b, c) >= 2 * batch * a * b * 4 == 134217728
    monkeypatch.setattr(rt.ops, "_STAGE1_BWD_GEMM_BYTES", 16 << 20)
    assert rt.ops.stage1_backward_route(batch, a, b, c) == "stream"
    params, flt, h, r, idc = _case(rt, n_ent, rank, batch, 55, torch.float32, n_subj=n_subj)
    cap = batch * a * b * 4 // 2
    max_pos = batch * flt.max_list
    stream_ws = lib.rtk_query_bwd_stream_workspace_bytes(batch, a, b, c)
    loss_ws = (lib.rtk_bce_stream_part_workspace_bytes(batch, n_ent, c, max_pos) + lib.rtk_workspace_bytes(0, batch, N_REL, a, b, c)
               + (1 << 20))
    saved = 3 * batch * c * 4 + lib.rtk_packed_query_bytes(0, batch, c) + batch * 8     # v, dv, dv * g, the planes, the loss rows
    grads = (a * b * c + N_REL * a + n_subj * b + n_ent * c) * 4                       # the fp32 gradients (autograd keeps them as .grad)
    design = stream_ws + loss_ws + saved + grads
    print(f"\n[stage-1 route] the design holds {design / 1e6:.1f} MB (stream workspace {stream_ws / 1e6:.1f}, loss workspace "
          f"{loss_ws / 1e6:.1f}, gradients {grads / 1e6:.1f}); cap {cap / 1e6:.1f} MB")
    assert design < cap
    ps = [p.clone().requires_grad_(True) for p in params]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=EPS)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.1f} MB; one (B, a*b) fp32 matrix is {batch * a * b * 4 / 1e6:.0f} MB")
    assert rise < cap
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in ps)
