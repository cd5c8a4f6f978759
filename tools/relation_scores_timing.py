#!/usr/bin/env python3
"""Wall-clock means (HIP events) of relation prediction, ops.pair_vectors and ops.score_relations, next to the
composition of older entry points that gives the same numbers through a (B, a*b) intermediate:

    x = O[t];  planes = pack_query_vectors(x);  W = score_packed_into(planes, core viewed as (a*b, c))   (B, a*b) fp32
    u = (W.view(B, a, b) * S[h][:, None, :]).sum(2);  p = score_packed_into(pack_query_vectors(u), R)

Shapes: WN18RR (a 10, b = c = 200, B 512, fp32, 22 relations) and FB15k-237 (a = b = c = 200, B 2048, bf16, 474
relations).  The two paths are timed alternately in one process, ROUNDS means of REPS calls each; the size of the
composition's intermediate is printed beside the times, and the largest difference between the two paths' u and p.
``--out FILE`` also writes the report there."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt                                   # noqa: E402

ROUNDS, REPS = 5, 300


def timed(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    lines = [f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating rounds, mean of {REPS} calls each, us per call"]
    g = torch.Generator(device="cuda").manual_seed(3)
    for name, (a, bc, B, n_ent, n_rel, dt) in (("WN18RR a 10, b = c = 200, B 512, fp32", (10, 200, 512, 40943, 22, torch.float32)),
                                               ("FB15k-237 a = b = c = 200, B 2048, bf16", (200, 200, 2048, 14541, 474, torch.bfloat16))):
        core = (torch.randn((a, bc, bc), device="cuda", generator=g) * (3.0 / (a * bc * bc) ** 0.5)).to(dt)
        R = torch.randn((n_rel, a), device="cuda", generator=g).to(dt)
        S = torch.randn((n_ent, bc), device="cuda", generator=g).to(dt)
        O = torch.randn((n_ent, bc), device="cuda", generator=g).to(dt)
        h = torch.randint(0, n_ent, (B,), device="cuda", generator=g)
        t = torch.randint(0, n_ent, (B,), device="cuda", generator=g)
        G2 = core.view(a * bc, bc)
        W = torch.empty((B, a * bc), dtype=torch.float32, device="cuda")
        P = torch.empty((B, n_rel), dtype=torch.float32, device="cuda")

        def comp_u():
            qp = rt.pack_query_vectors(O[t].float(), dt)
            rt.score_packed_into(qp, B, G2, W, sigmoid=False)
            return (W.view(B, a, bc) * S[h].float()[:, None, :]).sum(2)

        def comp_p():
            rt.score_packed_into(rt.pack_query_vectors(comp_u(), dt), B, R, P)
            return P

        def new_u():
            return rt.pair_vectors(core, S, O, h, t)

        def new_p():
            return rt.score_relations(core, R, S, O, h, t)

        with rt.index_check("off"), torch.no_grad():
            du = (new_u() - comp_u()).abs().max().item() / comp_u().abs().max().item()
            dp = (new_p() - comp_p()).abs().max().item()
            fns = (("pair_vectors", new_u), ("composition, u", comp_u), ("score_relations", new_p), ("composition, p", comp_p))
            for _, fn in fns:
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            res = {k: [] for k, _ in fns}
            for _ in range(ROUNDS):
                for k, fn in fns:
                    res[k].append(timed(fn))
        lines.append(f"\n{name}: the composition's (B, a*b) fp32 intermediate is {B * a * bc * 4 / 2 ** 20:.1f} MiB; "
                     f"pair_vectors' workspace is "
                     f"{rt._lib.load().rtk_pair_vectors_workspace_bytes(int(dt == torch.bfloat16), B, a, bc, bc) / 2 ** 20:.1f} MiB")
        lines.append(f"  largest |u_new - u_comp| / max |u| = {du:.2e}, largest |p_new - p_comp| = {dp:.2e}")
        for k, v in res.items():
            lines.append(f"  {k:18s} " + " ".join(f"{x:9.1f}" for x in v) + f"   mean {sum(v) / len(v):9.1f}  "
                         f"spread {100 * (max(v) - min(v)) / (sum(v) / len(v)):.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
