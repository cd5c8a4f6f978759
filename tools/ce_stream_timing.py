#!/usr/bin/env python3
"""Forward + backward and the no_grad forward of ce_loss_1vN in its two forms (stored logits / matrix_free=True), and
of bce_loss_1vN(matrix_free=True) in the same process, event-timed, with torch.cuda.max_memory_allocated: the shapes
and the method of tools/loss_stream_timing.py (WN18RR: N 40 943, rank (10, 200, 200), B 512; N = 1 000 000, rank
(10, 200, 200), B 4096).  Medians of --iters event-timed calls per form.  Kernel medians: run under
`rocprofv3 --kernel-trace --stats -- python tools/ce_stream_timing.py`.
  --shape wn18rr | big | both      --iters N"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gen  # noqa: E402
import r_tucker_amd as rt  # noqa: E402
from loss_stream_timing import SyntheticPairs, peak_of, timed  # noqa: E402

FORMS = (("ce  matrix     ", lambda: rt.ce_loss_1vN, False), ("ce  matrix-free", lambda: rt.ce_loss_1vN, True),
         ("bce matrix-free", lambda: rt.bce_loss_1vN, True))


def run(name, n_ent, n_rel, rank, B, flt, ids, warm, iters):
    core, R, S, O = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gen.make_params(n_ent, n_rel, rank, 322)]
    f = flt.features[ids]
    h, r = f[:, 0].contiguous(), f[:, 1].contiguous()

    def step(fn, mf):
        for p in (core, R, S, O):
            p.grad = None
        loss = fn(core, R, S, O, h, r, flt, ids, label_smoothing=0.1, matrix_free=mf)
        loss.backward()
        return loss

    def fwd(fn, mf):
        with torch.no_grad():
            return fn(core, R, S, O, h, r, flt, ids, label_smoothing=0.1, matrix_free=mf)

    print(f"== {name}: N {n_ent}, rank {rank}, B {B}; the matrix is {B * n_ent * 4 / 1e6:.0f} MB")
    res = {}
    for label, get, mf in FORMS:                             # the forms one after the other, one round: plain medians
        fn = get()
        res[label] = (timed(lambda: step(fn, mf), warm, iters), timed(lambda: fwd(fn, mf), warm, iters))
    for label, get, mf in FORMS:
        fn = get()
        t_step, t_fwd = res[label]
        print(f"  {label}: forward+backward {t_step:9.3f} ms  no_grad forward {t_fwd:9.3f} ms  backward (difference) "
              f"{t_step - t_fwd:9.3f} ms  peak over the live bytes {peak_of(lambda: step(fn, mf)):9.1f} MB  "
              f"loss {step(fn, mf).item():.6f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=("wn18rr", "big", "both"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.shape in ("wn18rr", "both"):
        from r_tucker_amd.data import Data, KG_dataset
        data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
        train = KG_dataset(data, data.train_data, label_smoothing=0.1)
        flt = rt.DeviceFilter(train, "cuda")
        run("WN18RR", len(data.entities), len(data.relations), (10, 200, 200), 512, flt,
            torch.arange(2000, 2000 + 512).cuda(), a.warmup, a.iters)
    if a.shape in ("big", "both"):
        n_ent, n_rel, B = 1_000_000, 22, 4096
        flt = rt.DeviceFilter(SyntheticPairs(n_ent, n_rel, B, 1), "cuda")
        run("1 M entities", n_ent, n_rel, (10, 200, 200), B, flt, torch.arange(B).cuda(), a.warmup, a.iters)
