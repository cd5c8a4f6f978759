"""The matrix-free 1-vs-all BCE loss on bf16 operands at the Python level (bce_loss_block_1vN and
ShardedEntityScorer.bce_loss_1vN over rtk_bce_stream_*_part_bf16): the whole range against the matrix form on the same
bf16 leaves, three blocks adding up, world size 1, no_grad, the empty batch, the refusals that stay, the shared-factor
model and peak memory."""
import numpy as np
import pytest
import torch

from r_tucker_amd.synthetic import make_params

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -7           # one ulp of a bf16 value g is at most 2^-7 |g|


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


def _case(rt, n_ent, rank, B, seed, eps=0.1, n_rel=7, n_subj=None, max_len=9):
    """bf16 parameters (the core scaled by 0.4: nothing saturates), a filter with one empty list, a batch of B items."""
    core, R, S, O = make_params(n_ent, n_rel, rank, seed)
    n_subj = n_subj or n_ent
    rng = np.random.default_rng(seed)
    n_pairs = max(B, 1)
    pairs = [(int(s), int(r_)) for s, r_ in zip(rng.permutation(n_subj)[:n_pairs], rng.integers(0, n_rel, n_pairs))]
    lists = [np.unique(rng.integers(0, n_ent, int(rng.integers(1, max_len)))).tolist() for _ in pairs]
    lists[0] = []
    ds = _Pairs(pairs, lists, n_ent, eps)
    flt = rt.DeviceFilter(ds, "cuda")
    ids = rng.permutation(n_pairs)[:B].astype(np.int64)
    params = [torch.from_numpy(np.ascontiguousarray(x)).cuda().bfloat16() for x in (core * 0.4, R, S[:n_subj], O)]
    h = torch.from_numpy(ds.features[ids, 0].copy()).cuda()
    r = torch.from_numpy(ds.features[ids, 1].copy()).cuda()
    return params, flt, h, r, torch.from_numpy(ids).cuda()


def _leaves(params):
    return [p.clone().requires_grad_(True) for p in params]


def _run(loss_fn, params, weight=3.0):
    ps = _leaves(params)
    loss = loss_fn(ps)
    (loss * weight).backward()
    return loss.detach(), [p.grad for p in ps]


def _close(a, b):
    """The loss bound of tests/test_gpu_loss_stream.py."""
    return abs(float(a) - float(b)) <= 2e-6 * max(1.0, abs(float(b)))


@pytest.mark.parametrize("smode", ["fast", "exact"])
@pytest.mark.parametrize("rank", [(3, 32, 32), (3, 512, 512)], ids=["c32", "c512"])
def test_whole_range_against_the_matrix_form(rt, rank, smode):
    """bce_loss_block_1vN on (0, n_ent) against bce_loss_1vN(matrix_free=False) on the same bf16 leaves: the loss
    within 2e-6 max(1, |loss|); every gradient is bf16 and the two forms differ by at most 2^-7 max|g| per tensor -- both
    compute the same quantity to better than 2^-20 of its max-norm in fp32, so after the final rounding they differ by
    at most one bf16 ulp."""
    n_ent, B, eps = 3003, 70, 0.1
    params, flt, h, r, idc = _case(rt, n_ent, rank, B, 41, eps)
    l_blk, g_blk = _run(lambda ps: rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps,
                                                         sigmoid_mode=smode), params)
    l_mat, g_mat = _run(lambda ps: rt.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=eps), params)
    print(f"\n[loss stream bf16] rank {rank} {smode}: loss {float(l_blk):.8f} (block) {float(l_mat):.8f} (matrix)")
    assert l_blk.dtype == torch.float32 and _close(l_blk, l_mat)
    for name, a, b in zip(("core", "R", "S", "O"), g_blk, g_mat):
        assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape, name
        top = b.float().abs().max().item()
        err = (a.float() - b.float()).abs().max().item()
        print(f"  {name}: max|g| {top:.3e}, max difference {err:.3e} = {err / top / BF16_ULP:.3f} x 2^-7 max|g|")
        assert top > 0 and err <= BF16_ULP * top, name


def test_three_blocks_add_up(rt):
    """all_reduce=None: the blocks' shares.  The losses sum to the whole-range loss (2e-6 max(1, |loss|)); the shares
    of the core / R / S gradients, each rounded to bf16 once (half an ulp: at most 2^-8 of its max-norm) as the
    whole-range gradient is, sum to it within 2^-8 (sum_i max|g_i| + max|g|) + 2^-20 max|g| for the fp32 sums' order; the O_loc gradients
    concatenate to the whole-range one within one bf16 ulp, 2^-7 max|g|."""
    n_ent, B, eps, rank = 3003, 70, 0.1, (3, 32, 32)
    params, flt, h, r, idc = _case(rt, n_ent, rank, B, 43, eps)
    l_all, g_all = _run(lambda ps: rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps), params)
    cuts = [0, 1000, 1501, n_ent]
    loss, shares, rows_of_gO = 0.0, [], []
    for lo, hi in zip(cuts, cuts[1:]):
        blk = params[:3] + [params[3][lo:hi].contiguous()]
        l_b, g_b = _run(lambda ps: rt.bce_loss_block_1vN(*ps, lo, n_ent, h, r, flt, idc, label_smoothing=eps), blk)
        loss += float(l_b)
        shares.append(g_b[:3])
        rows_of_gO.append(g_b[3])
    assert _close(loss, l_all)
    for k, name in enumerate(("core", "R", "S")):
        total = sum(s[k].float() for s in shares)
        top = g_all[k].float().abs().max().item()
        tol = 2.0 ** -8 * (sum(s[k].float().abs().max().item() for s in shares) + top) + 2.0 ** -20 * top
        assert (total - g_all[k].float()).abs().max().item() <= tol, name
    gO = torch.cat(rows_of_gO)
    top = g_all[3].float().abs().max().item()
    assert gO.dtype == torch.bfloat16 and (gO.float() - g_all[3].float()).abs().max().item() <= BF16_ULP * top


def test_world_size_one_no_grad_and_the_empty_batch(rt):
    n_ent, B, eps, rank = 3003, 70, 0.1, (3, 32, 32)
    params, flt, h, r, idc = _case(rt, n_ent, rank, B, 45, eps)
    block = _run(lambda ps: rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps), params)
    sc = rt.ShardedEntityScorer(n_ent)
    assert sc.world == 1 and sc.shards.n_loc == n_ent
    shard = _run(lambda ps: sc.bce_loss_1vN(*ps, h, r, flt, idc, label_smoothing=eps), params)
    assert torch.equal(block[0], shard[0])
    for a, b in zip(block[1], shard[1]):
        assert a.dtype == b.dtype == torch.bfloat16 and torch.equal(a, b)
    with torch.no_grad():                                   # the loss-only forward: no dv, the same loss bits
        ps = _leaves(params)
        loss = rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps)
    assert not loss.requires_grad and torch.equal(loss, block[0])
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    l0, g0 = _run(lambda ps: rt.bce_loss_block_1vN(*ps, 0, n_ent, none, none, flt, none, label_smoothing=eps), params)
    assert float(l0) == 0.0
    for p, g in zip(params, g0):
        assert g.dtype == torch.bfloat16 and g.shape == p.shape and not g.any()


def test_gO_in_row_blocks_is_gO(rt, monkeypatch):
    """The gradient of O_loc goes through an fp32 staging buffer, a sub-block of rows per call: three calls give what
    one call gives, within one bf16 ulp of the max-norm (the ordered scatter's windows fall elsewhere)."""
    n_ent, B, eps, rank = 3003, 70, 0.1, (3, 32, 32)
    params, flt, h, r, idc = _case(rt, n_ent, rank, B, 51, eps)
    loss_fn = lambda ps: rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps)  # noqa: E731
    assert rt.ops._GO_STAGE_BYTES >= n_ent * 32 * 4
    l_one, g_one = _run(loss_fn, params)
    monkeypatch.setattr(rt.ops, "_GO_STAGE_BYTES", 1024 * 32 * 4)           # 1024 rows per call: 1024 + 1024 + 955
    l_three, g_three = _run(loss_fn, params)
    assert torch.equal(l_one, l_three)
    for a, b in zip(g_one[:3], g_three[:3]):
        assert torch.equal(a, b)
    top = g_one[3].float().abs().max().item()
    assert g_three[3].dtype == torch.bfloat16 and g_three[3].any()
    assert (g_three[3].float() - g_one[3].float()).abs().max().item() <= BF16_ULP * top


def test_refusals(rt):
    n_ent, B, eps, rank = 500, 16, 0.1, (3, 32, 32)
    params, flt, h, r, idc = _case(rt, n_ent, rank, B, 47, eps)
    for k in range(4):                                      # mixed dtypes, whichever operand differs
        for mixed in ([p.float() if i == k else p for i, p in enumerate(params)],
                      [p if i == k else p.float() for i, p in enumerate(params)]):
            with pytest.raises(RuntimeError, match="share one dtype"):
                rt.bce_loss_block_1vN(*mixed, 0, n_ent, h, r, flt, idc, label_smoothing=eps)
    # what keeps refusing bf16: the whole-matrix entry and the cross-entropy losses
    with pytest.raises(RuntimeError, match="float32 operands only"):
        rt.bce_loss_1vN(*params, h, r, flt, idc, label_smoothing=eps, matrix_free=True)
    for matrix_free in (False, True):
        with pytest.raises(RuntimeError, match="float32 operands only"):
            rt.ce_loss_1vN(*params, h, r, flt, idc, label_smoothing=eps, matrix_free=matrix_free)
    with pytest.raises(RuntimeError, match="float32 operands only"):
        rt.ce_loss_block_1vN(*params, 0, n_ent, h, r, flt, idc, label_smoothing=eps)
    # outside the bf16 range: c % 8 != 0, c > 512
    for c in (20, 520):
        core, R, S, O = [torch.from_numpy(x).cuda().bfloat16() for x in make_params(n_ent, 7, (3, c, c), 3)]
        with pytest.raises(RuntimeError, match="outside the matrix-free range of bf16"):
            rt.bce_loss_block_1vN(core, R, S, O, 0, n_ent, h, r, flt, idc, label_smoothing=eps)
    with pytest.raises(RuntimeError, match="is not a part of"):
        rt.bce_loss_block_1vN(*params, 1, n_ent, h, r, flt, idc, label_smoothing=eps)


def test_the_shared_factor_model_gets_both_gradients(rt):
    """S and O the same tensor: its gradient is the (bf16) sum of the two the separate leaves get."""
    n_ent, B, eps, rank = 3003, 70, 0.1, (3, 32, 32)
    (core, R, S, _), flt, h, r, idc = _case(rt, n_ent, rank, B, 49, eps)
    _, (g_core, g_R, g_S, g_O) = _run(lambda ps: rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps),
                                      [core, R, S, S])
    ps = _leaves([core, R, S])
    (rt.bce_loss_block_1vN(ps[0], ps[1], ps[2], ps[2], 0, n_ent, h, r, flt, idc, label_smoothing=eps) * 3.0).backward()
    assert torch.equal(ps[0].grad, g_core) and torch.equal(ps[1].grad, g_R)
    assert g_S.any() and g_O.any() and torch.equal(ps[2].grad, g_S + g_O)


def test_no_batch_times_entities_allocation(rt):
    """N 200 000, c 64, B 2048 in bf16 (the bf16 score matrix would be 819 MB): forward + backward raise the peak by less
    than B N 2 / 8.  First the sum of what the design holds at its peak -- the workspace, what is saved between
    forward and backward, the bf16 gO with the fp32 staging buffer of its rows and the stage-1 backward's tensors -- is
    shown to fit."""
    n_ent, B, eps, rank, n_subj = 200_000, 2048, 0.1, (4, 64, 64), 4096
    a, b, c = rank
    params, flt, h, r, idc = _case(rt, n_ent, rank, B, 5, eps, n_subj=n_subj)
    cap = B * n_ent * 2 // 8
    lib = rt._lib.load()
    max_pos = B * flt.max_list
    ws = max(lib.rtk_bce_stream_bf16_workspace_bytes(B, n_ent, c, max_pos), lib.rtk_workspace_bytes(1, B, 7, a, b, c),
             1 << 20)
    saved = B * c * 4 * 2 + lib.rtk_packed_query_bytes(1, B, c) + B * 8            # v, dv, the planes, the loss rows
    stage = min(rt.ops._GO_STAGE_BYTES, n_ent * c * 4)
    assert stage < n_ent * c * 4, "gO is written through the fp32 staging buffer in more than one call"
    g_o = n_ent * c * 2 + stage                                                    # gO in bf16 and the fp32 rows of a call
    small = (a * b * c + 7 * a + n_subj * b) * (4 + 4 + 2) + B * c * 4 + lib.rtk_query_bwd_workspace_bytes(B, a, b, c)
    design = ws + saved + g_o + small
    print(f"\n[loss stream bf16] the design holds {design / 1e6:.1f} MB (workspace {ws / 1e6:.1f}, gO {g_o / 1e6:.1f}); "
          f"cap {cap / 1e6:.1f} MB")
    assert design < cap
    ps = _leaves(params)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = rt.bce_loss_block_1vN(*ps, 0, n_ent, h, r, flt, idc, label_smoothing=eps)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise / 1e6:.1f} MB; the bf16 score matrix is {B * n_ent * 2 / 1e6:.0f} MB")
    assert rise < cap
    assert ps[3].grad.shape == (n_ent, c) and ps[3].grad.dtype == torch.bfloat16 and torch.isfinite(loss)
