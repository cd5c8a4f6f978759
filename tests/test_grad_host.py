"""The host pieces every differentiable op of ops.py shares, and the one body of the two model flavours, on the CPU:
the zero gradients of an empty batch, the fp32 view of the operands and the cast back, "does any operand want a
gradient", the row pitch, the spent guard of the stored-matrix losses; the five object-query methods of both model
classes are one implementation and their state_dict keys are the reference's."""
import types

import pytest
import torch

import r_tucker_amd as rt
from r_tucker_amd import ops


def _ctx(saved, needs):
    return types.SimpleNamespace(saved_tensors=tuple(saved), needs_input_grad=tuple(needs))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("needs", [(True, True, True, True), (False, True, False, True), (True, False, False, False),
                                   (False, False, False, False)])
def test_zero_batch_grads_follow_needs_input_grad(dtype, needs):
    core, R, S, O = (torch.ones(s, dtype=dtype) for s in ((3, 8, 8), (4, 3), (50, 8), (50, 8)))
    extra = (torch.zeros(0, dtype=torch.int64), None, torch.zeros((0, 50)))      # what else a forward saved
    for n_other in (2, 5, 14):
        got = ops._zero_batch_grads(_ctx((core, R, S, O) + extra, needs + (False,) * n_other))
        assert len(got) == 4 + n_other and all(g is None for g in got[4:])
        for g, t, n in zip(got, (core, R, S, O), needs):
            if not n:
                assert g is None
            else:
                assert g.shape == t.shape and g.dtype == t.dtype and g.device == t.device
                assert not g.any()


def test_f32_view_and_cast_back():
    f = [torch.randn(3, 4), torch.randn(5, 3)]
    assert all(a is b for a, b in zip(ops._f32(*f), f)), "fp32 operands are taken as they are"
    grads = (f[0], None, f[1])
    back = ops._grads_like(grads, torch.float32)
    assert isinstance(back, tuple) and back[1] is None and back[0] is f[0] and back[2] is f[1]
    b = [t.to(torch.bfloat16) for t in f]
    up = ops._f32(*b)
    assert all(u.dtype == torch.float32 and torch.equal(u, t.float()) for u, t in zip(up, b))
    down = ops._grads_like((up[0], None, up[1]), torch.bfloat16)
    assert down[1] is None and all(d.dtype == torch.bfloat16 for d in (down[0], down[2]))
    assert torch.equal(down[0], b[0]) and torch.equal(down[2], b[1]), "bf16 -> fp32 -> bf16 is the identity"


def test_wants_grad():
    a, b = torch.zeros(2, requires_grad=True), torch.zeros(2)
    assert ops._wants_grad(b, a) and ops._wants_grad(a)
    assert not ops._wants_grad(b, b) and not ops._wants_grad(b, None, [1, 2]) and not ops._wants_grad()
    with torch.no_grad():
        assert not ops._wants_grad(a, b)
    assert ops._wants_grad(a, b)


def test_row_pitch():
    buf = torch.zeros(4, 160)
    assert ops._ld(buf[:, :130]) == 160 and ops._ld(buf) == 160
    assert ops._ld(buf[:1, :130]) == 130 and ops._ld(buf[:0, :130]) == 130        # at most one row: the column count
    assert ops._ld(torch.zeros(1, 7).expand(5, 7)) == 0                           # one row shared by the batch


def test_spent_guard_keeps_the_error_texts():
    ctx = types.SimpleNamespace()
    ops._spend(ctx, "bce_loss_1vN", "scores")
    with pytest.raises(RuntimeError) as e:
        ops._spend(ctx, "bce_loss_1vN", "scores")
    assert str(e.value) == "bce_loss_1vN: backward called twice (the saved scores are overwritten by the first pass)"
    ctx = types.SimpleNamespace()
    ops._spend(ctx, "ce_loss_1vN", "logits")
    with pytest.raises(RuntimeError) as e:
        ops._spend(ctx, "ce_loss_1vN", "logits")
    assert str(e.value) == "ce_loss_1vN: backward called twice (the saved logits are overwritten by the first pass)"


METHODS = ("forward", "score_candidates", "score_triples", "predict", "rank_objects")


def test_both_flavours_share_one_body():
    A, S = rt.AsymmetricR_TuckER, rt.SymmetricR_TuckER
    from r_tucker_amd.model.asymmetric.R_TuckER import R_TuckER as A2
    from r_tucker_amd.model.symmetric.R_TuckER import R_TuckER as S2
    assert A is A2 and S is S2 and A.__name__ == S.__name__ == "R_TuckER"
    for name in METHODS:
        assert getattr(A, name) is getattr(S, name), name
        assert name not in vars(A) and name not in vars(S), name
    for cls in (A, S):                                   # the flavour keeps its constructor, init() and the two hooks
        assert {"__init__", "init", "_operands_of", "_relation_operands"} <= set(vars(cls))


def test_state_dict_keys_and_hooks():
    a = rt.AsymmetricR_TuckER((7, 3), (2, 4, 4))
    s = rt.SymmetricR_TuckER((7, 3), (2, 4, 4))
    assert list(a.state_dict()) == ["core", "S.weight", "R.weight", "O.weight"]
    assert list(s.state_dict()) == ["core", "E.weight", "R.weight"]
    got = a._relation_operands()
    assert all(x is y for x, y in zip(got, (a.core, a.R.weight, a.S.weight, a.O.weight)))
    got = s._relation_operands()
    assert all(x is y for x, y in zip(got, (s.core, s.R.weight, s.E.weight, s.E.weight)))
    T = rt.Tucker(a.core.data, [a.R.weight, a.S.weight, a.O.weight])
    got = a._operands_of(T)
    assert all(x is y for x, y in zip(got, (T.core, T.factors[0], T.factors[1], T.factors[2])))
    Ts = rt.SFTucker(s.core.data, [s.R.weight], 2, s.E.weight)
    got = s._operands_of(Ts)
    assert got[0] is Ts.core and got[1] is Ts.regular_factors[0] and got[2] is Ts.shared_factor and got[3] is Ts.shared_factor
