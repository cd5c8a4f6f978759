"""Every differentiable op at B = 0 with every operand requiring a gradient: the forward has the shape its siblings
give (or is exactly 0 for a loss), backward() gives all-zero gradients of each operand's shape and dtype, and the
device error word stays clear.  50 entities, 4 relations, rank (3, 8, 8), fp32; asymmetric and S is O."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

N_ENT, N_REL, RANK = 50, 4, (3, 8, 8)


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _leaves(shared):
    g = torch.Generator().manual_seed(50)
    shapes = (RANK, (N_REL, RANK[0]), (N_ENT, RANK[1])) + (() if shared else ((N_ENT, RANK[2]),))
    leaves = [(0.5 * torch.randn(s, generator=g)).cuda().requires_grad_(True) for s in shapes]
    return leaves, (leaves + [leaves[2]] if shared else leaves)      # shared: the one entity matrix as S and as O


def _empty():
    return torch.zeros(0, dtype=torch.int64, device="cuda")


def _flt():
    t = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda")  # noqa: E731
    return SimpleNamespace(slot_of_item=t([0, 1]), pair_ptr=t([0, 2, 3]), pair_obj=t([1, 5, 7]), max_list=2)


CASES = {
    "score_1vN sigmoid": (lambda rt, p: rt.score_1vN(*p, _empty(), _empty(), sigmoid=True), (0, N_ENT)),
    "score_1vN logits": (lambda rt, p: rt.score_1vN(*p, _empty(), _empty(), sigmoid=False), (0, N_ENT)),
    "bce_loss_1vN matrix": (lambda rt, p: rt.bce_loss_1vN(*p, _empty(), _empty(), _flt(), _empty(), 0.1), ()),
    "bce_loss_1vN matrix_free": (lambda rt, p: rt.bce_loss_1vN(*p, _empty(), _empty(), _flt(), _empty(), 0.1,
                                                               matrix_free=True), ()),
    "ce_loss_1vN matrix": (lambda rt, p: rt.ce_loss_1vN(*p, _empty(), _empty(), _flt(), _empty(), 0.1), ()),
    "ce_loss_1vN matrix_free": (lambda rt, p: rt.ce_loss_1vN(*p, _empty(), _empty(), _flt(), _empty(), 0.1,
                                                             matrix_free=True), ()),
    "score_candidates K=3": (lambda rt, p: rt.score_candidates(*p, _empty(), _empty(),
                                                               torch.zeros((0, 3), dtype=torch.int64, device="cuda")), (0, 3)),
    "relation_logits": (lambda rt, p: rt.relation_logits(*p, _empty(), _empty()), (0, N_REL)),
}


@pytest.mark.parametrize("shared", [False, True], ids=["asym", "S_is_O"])
@pytest.mark.parametrize("name", list(CASES))
def test_empty_batch_gives_zero_gradients(rt, name, shared):
    call, shape = CASES[name]
    leaves, operands = _leaves(shared)
    out = call(rt, operands)
    assert out.requires_grad and out.dtype == torch.float32 and out.is_cuda
    assert tuple(out.shape) == shape
    if shape == ():
        assert out.item() == 0.0
        out.backward()
    else:
        out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    for leaf in leaves:
        assert leaf.grad is not None
        assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == leaf.dtype and leaf.grad.device == leaf.device
        assert not leaf.grad.any()
    rt.check_device_errors()
