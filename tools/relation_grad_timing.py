#!/usr/bin/env python3
"""Wall-clock means (HIP events) of training relation prediction: ops.relation_logits forward plus backward, the three
new kernels of its backward each on its own (rtk_pair_rows_f32, rtk_core_outer_f32, rtk_scatter_rows_f32), and the same
gradients taken by torch autograd through the einsum form

    z = einsum("ijk,dj,dk,ri->dr", core, S[h], O[t], R)

on the same GPU, with the peak memory of each.  Shapes: WN18RR (a 10, b = c = 200, B 512, 11 relations) and
(a = b = c = 200, B 2048, 237 relations), fp32.  The paths are timed alternately in one process, ROUNDS means of REPS
calls each after a warm-up.  ``--out FILE`` also writes the report there."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt                                   # noqa: E402

ROUNDS, REPS, WARM = 5, 50, 5


def timed(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3      # us


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    lines = [f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating rounds, mean of {REPS} calls each after {WARM} "
             "warm-up calls, us per call; peak = memory allocated above the operands during one call, MiB"]
    g = torch.Generator(device="cuda").manual_seed(3)
    for name, (a, bc, B, n_ent, n_rel) in (("WN18RR a 10, b = c = 200, B 512, 11 relations", (10, 200, 512, 40943, 11)),
                                           ("a = b = c = 200, B 2048, 237 relations", (200, 200, 2048, 14541, 237))):
        rnd = lambda *s: torch.randn(s, device="cuda", generator=g)
        core = (rnd(a, bc, bc) * (3.0 / (a * bc * bc) ** 0.5)).requires_grad_()
        R, S, O = rnd(n_rel, a).requires_grad_(), rnd(n_ent, bc).requires_grad_(), rnd(n_ent, bc).requires_grad_()
        h = torch.randint(0, n_ent, (B,), device="cuda", generator=g)
        t = torch.randint(0, n_ent, (B,), device="cuda", generator=g)
        dZ = rnd(B, n_rel)
        du, Sh, Ot = rnd(B, a), S.detach()[h], O.detach()[t]
        Gd, Od = core.detach(), O.detach()
        rows = rt.pair_rows(Gd, Od, t, du)

        def new():
            return torch.autograd.grad(rt.relation_logits(core, R, S, O, h, t), (core, R, S, O), dZ)

        def einsum():
            z = torch.einsum("ijk,dj,dk,ri->dr", core, S[h], O[t], R)
            return torch.autograd.grad(z, (core, R, S, O), dZ)

        fns = (("relation_logits fwd+bwd", new), ("einsum autograd fwd+bwd", einsum),
               ("score_relations (fwd only)", lambda: rt.score_relations(Gd, R.detach(), S.detach(), Od, h, t, sigmoid=False)),
               ("rtk_pair_rows_f32", lambda: rt.pair_rows(Gd, Od, t, du)),
               ("rtk_core_outer_f32", lambda: rt.core_outer(du, Sh, Ot)),
               ("rtk_scatter_rows_f32", lambda: rt.scatter_rows(h, rows, n_ent)))
        with rt.index_check("off"):
            err = [((x - y).abs().max() / y.abs().max()).item() for x, y in zip(new(), einsum())]
            for _, fn in fns:
                for _ in range(WARM):
                    fn()
            peaks = {k: peak_of(fn) for k, fn in fns}
            res = {k: [] for k, _ in fns}
            for _ in range(ROUNDS):
                for k, fn in fns:
                    res[k].append(timed(fn))
        flop = 2.0 * B * a * bc * bc
        lines.append(f"\n{name}: a (B, a*b) fp32 buffer would be {B * a * bc * 4 / 2 ** 20:.1f} MiB; rtk_pair_rows_f32's workspace "
                     f"is {rt._lib.load().rtk_pair_rows_workspace_bytes(B, a, bc, bc) / 2 ** 20:.1f} MiB")
        lines.append("  largest |g_new - g_einsum| / max |g| (core, R, S, O) = " + ", ".join(f"{e:.1e}" for e in err))
        for k, v in res.items():
            m = sum(v) / len(v)
            lines.append(f"  {k:28s} " + " ".join(f"{x:9.1f}" for x in v) + f"   mean {m:9.1f}  spread "
                         f"{100 * (max(v) - min(v)) / m:.1f} %  peak {peaks[k]:8.1f}")
        for k in ("rtk_pair_rows_f32", "rtk_core_outer_f32"):
            m = sum(res[k]) / len(res[k])
            lines.append(f"  {k}: {flop / 1e6:.0f} MFLOP of the product itself -> {flop / m / 1e6:.2f} TFLOP/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
