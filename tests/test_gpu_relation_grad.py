"""GPU tests of relation_logits / relation_ce_loss: the forward has the bits of score_relations(sigmoid=False), and the
four gradients of a random dZ lie within the bounds of the float64 model (tests/relation_grad_model.py), for fp32 and
bf16 operands, the symmetric model, B = 1 and B = 0, one operand at a time, and bit for bit on a second run."""
import numpy as np
import pytest
import torch

import relation_grad_model as gm
import relation_model as rm

pytestmark = pytest.mark.gpu

NAMES = ("core", "R", "S", "O")


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import r_tucker_amd
    r_tucker_amd._lib.load()
    return r_tucker_amd


def _params(case, bf16, needs=NAMES):
    out = {}
    for n in NAMES:
        t = torch.from_numpy(case[n]).cuda()
        out[n] = (t.bfloat16() if bf16 else t).requires_grad_(n in needs)
    return out


def _rounded(case, bf16):
    return {n: (rm.bf16_round(case[n]) if bf16 and n in NAMES else case[n]) for n in case}


def _backward(rt, p, h, t, dZ, symmetric=False):
    z = rt.relation_logits(p["core"], p["R"], p["S"], p["S"] if symmetric else p["O"], h, t)
    grads = torch.autograd.grad(z, [p[n] for n in NAMES[:3 if symmetric else 4] if p[n].requires_grad], dZ)
    names = [n for n in NAMES[:3 if symmetric else 4] if p[n].requires_grad]
    return z, dict(zip(names, grads))


def _check(grads, val, tau, label):
    for n, g in grads.items():
        key = "E" if n == "S" and "E" in val else n
        assert g.shape == val[key].shape
        err = np.abs(g.float().cpu().numpy() - val[key])
        print(f"{label} g{key}: max |dg| / tau = {np.max(err / np.maximum(tau[key], 1e-300)):.2e}")
        assert np.all(err <= tau[key]), (label, key)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["asym", "sym"])
def test_gradients_against_float64(rt, bf16, symmetric):
    case = _rounded(gm.grad_case(), bf16)
    p = _params(case, bf16)
    h, t, dZ = (torch.from_numpy(case[n]).cuda() for n in ("h", "t", "dZ"))
    z, grads = _backward(rt, p, h, t, dZ, symmetric)
    O = case["S"] if symmetric else case["O"]
    with torch.no_grad():
        ref = rt.score_relations(p["core"], p["R"], p["S"], p["S"] if symmetric else p["O"], h, t, sigmoid=False)
    assert z.dtype == torch.float32 and torch.equal(z.detach(), ref)
    assert all(g.dtype == p[n].dtype for n, g in grads.items())
    val, tau = gm.grad_bounds(case["core"], case["R"], case["S"], O, case["h"], case["t"], case["dZ"], symmetric, bf16)
    _check(grads, val, tau, f"{'bf16' if bf16 else 'f32'} {'sym' if symmetric else 'asym'}")
    again = _backward(rt, p, h, t, dZ, symmetric)[1]
    assert all(torch.equal(grads[n], again[n]) for n in grads)


@pytest.mark.parametrize("B", [1, 0])
def test_small_batches(rt, B):
    case = gm.grad_case(B=max(B, 1), seed=2)
    if B == 0:
        case = {n: (v[:0] if n in ("h", "t", "dZ", "rel") else v) for n, v in case.items()}
    p = _params(case, False)
    h, t, dZ = (torch.from_numpy(case[n]).cuda() for n in ("h", "t", "dZ"))
    z, grads = _backward(rt, p, h, t, dZ)
    assert z.shape == (B, case["R"].shape[0])
    if B == 0:
        assert all(g.shape == p[n].shape and torch.all(g == 0) for n, g in grads.items())
        return
    val, tau = gm.grad_bounds(*[case[n] for n in ("core", "R", "S", "O", "h", "t", "dZ")])
    _check(grads, val, tau, "B=1")


@pytest.mark.parametrize("only", NAMES)
def test_one_operand_at_a_time(rt, only):
    case = gm.grad_case()
    h, t, dZ = (torch.from_numpy(case[n]).cuda() for n in ("h", "t", "dZ"))
    full = _backward(rt, _params(case, False), h, t, dZ)[1]
    one = _backward(rt, _params(case, False, (only,)), h, t, dZ)[1]
    assert list(one) == [only] and torch.equal(one[only], full[only])


def test_ce_loss_and_models(rt):
    case = gm.grad_case()
    p = _params(case, False)
    h, t, rel = (torch.from_numpy(case[n]).cuda() for n in ("h", "t", "rel"))
    z64, tau_z, _ = rm.z_bounds(case["core"], case["R"], case["S"], case["O"], case["h"], case["t"], False)
    for ls in (0.0, 0.1):
        loss = rt.relation_ce_loss(p["core"], p["R"], p["S"], p["O"], h, t, rel, label_smoothing=ls)
        want = torch.nn.functional.cross_entropy(torch.from_numpy(z64), torch.from_numpy(case["rel"]), label_smoothing=ls)
        # a mean of B terms, each 1-Lipschitz in the logits' largest error (the softmax weights add up to 1)
        assert abs(loss.item() - want.item()) <= tau_z.max(), (ls, loss.item(), want.item(), tau_z.max())
        loss.backward()
        assert all(p[n].grad is not None and torch.isfinite(p[n].grad).all() and p[n].grad.abs().max() > 0 for n in NAMES)
    for cls, sym in ((rt.AsymmetricR_TuckER, False), (rt.SymmetricR_TuckER, True)):
        m = cls((case["S"].shape[0], case["R"].shape[0]), tuple(case["core"].shape)).cuda()
        with torch.no_grad():
            m.core.normal_(0.0, 0.5)                                    # (the models start from a zero core)
        z = m.relation_logits(h, t)
        assert z.shape == (h.numel(), case["R"].shape[0]) and z.requires_grad
        with torch.no_grad():
            assert torch.equal(z.detach(), rt.score_relations(*m._relation_operands(), h, t, sigmoid=False))
        torch.nn.functional.cross_entropy(z, rel).backward()
        params = [m.core, m.R.weight] + ([m.E.weight] if sym else [m.S.weight, m.O.weight])
        assert all(q.grad is not None and torch.isfinite(q.grad).all() and q.grad.abs().max() > 0 for q in params)
