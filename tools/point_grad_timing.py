#!/usr/bin/env python3
"""One training step (``fit`` + ``step`` of RSGD with momentum) on WN18RR at the README rank (10,200,200), B 512, fp32,
in the three forms of the Riemannian gradient:

    construct + matrix form   the loss differentiated at the doubled-rank construct, core (20,400,400): the default
    point + matrix form       one backward at the point's own rank (train_cfg.grad_at=point)
    point + matrix-free       the same without the (B, n_ent) score matrix (train_cfg.matrix_free=true)

Each row has its own model (same seed, same first batches) and optimizer and goes through the driver's own step
object.  After a warm-up the rows are timed in alternating rounds, every step between two device synchronisations;
reported: the median over all timed steps, the range of the per-round medians, the peak memory rise of a step over
what is allocated between steps, and the loss of the first step (the three forms start from the same point).  A last
pass synchronises between ``fit`` and ``step`` to show how the time divides and what ``fit`` alone allocates (the
retraction in ``step`` works on the doubled-rank construct in every form).

    python tools/point_grad_timing.py [--rounds 5] [--steps 20] [--warmup 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (("construct + matrix form", "construct", False), ("point + matrix form", "point", False),
        ("point + matrix-free", "point", True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per row and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timings are taken on the GPU only"

    import r_tucker_amd as rt
    from configs.base_config import wn18rr_readme_config
    from r_tucker_amd import driver, ops
    from r_tucker_amd.data import Data, KG_dataset

    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    train = KG_dataset(data, data.train_data, label_smoothing=0.1)
    flt = rt.DeviceFilter(train, "cuda")
    n = flt.features.shape[0]
    perm = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(322))

    rows = []
    for name, grad_at, matrix_free in ROWS:
        cfg = wn18rr_readme_config()
        cfg.train_cfg.grad_at, cfg.train_cfg.matrix_free = grad_at, matrix_free
        tc = cfg.train_cfg
        torch.manual_seed(322)
        model = rt.AsymmetricR_TuckER((len(data.entities), len(data.relations)), cfg.model_cfg.manifold_rank)
        model.init()
        model.cuda()
        opt = driver.define_optimizer(model, cfg, "asymmetric", "rsgd")
        step = driver._captured_step(model, opt, flt, tc.train_batch_size, tc.label_smoothig, tc.loss, tc.matrix_free)
        step.begin_epoch(tc.base_regularization_coeff)
        rows.append({"name": name, "step": step, "opt": opt, "B": tc.train_batch_size, "next": 0, "times": [],
                     "round_medians": [], "rise": 0, "first_loss": None})

    def one(row):
        b, B = row["next"], row["B"]
        row["next"] = (b + 1) % (n // B)
        ids = perm[b * B:(b + 1) * B]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row["step"].run(ids)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def split(row):
        """One step with ``fit`` and ``step`` synchronised apart: (fit s, step s, peak rise of fit alone)."""
        b, B, st = row["next"], row["B"], row["step"]
        row["next"] = (b + 1) % (n // B)
        ids = perm[b * B:(b + 1) * B]
        f = flt.features[ids]
        loss_fn = st._loss_fn(st.model, f[:, 0].contiguous(), f[:, 1].contiguous(), flt, ids, st.ls, st.reg)
        x_k = st._extract(st.model)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        st.opt.fit(loss_fn, x_k)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rise = torch.cuda.max_memory_allocated() - before
        st.opt.step()
        torch.cuda.synchronize()
        return t1 - t0, time.perf_counter() - t1, rise

    with ops.index_check("deferred"):
        for row in rows:
            for i in range(args.warmup):
                one(row)
                if i == 0:
                    row["first_loss"] = float(row["opt"].loss)
        for _ in range(args.rounds):
            for row in rows:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                ts = [one(row) for _ in range(args.steps)]
                row["rise"] = max(row["rise"], torch.cuda.max_memory_allocated() - before)
                row["times"] += ts
                row["round_medians"].append(statistics.median(ts))
        for row in rows:
            parts = [split(row) for _ in range(args.steps)]
            row["fit"], row["opt_step"] = (statistics.median(p[i] for p in parts) for i in (0, 1))
            row["fit_rise"] = max(p[2] for p in parts)
    ops.check_device_errors()

    lines = [f"WN18RR, rank (10,200,200), B 512, RSGD with momentum, fp32, {torch.cuda.get_device_name(0)}",
             f"fit + step between device synchronisations; {args.warmup} warm-up steps, {args.rounds} alternating rounds of "
             f"{args.steps} steps per row",
             f"{'form':<26}{'median ms/step':>16}{'round medians ms':>22}{'peak rise MB':>14}{'first loss':>14}"]
    base = statistics.median(rows[0]["times"])
    for row in rows:
        med = statistics.median(row["times"])
        lo, hi = min(row["round_medians"]), max(row["round_medians"])
        lines.append(f"{row['name']:<26}{med * 1e3:>16.3f}{f'{lo * 1e3:.3f} .. {hi * 1e3:.3f}':>22}{row['rise'] / 1e6:>14.1f}"
                     f"{row['first_loss']:>14.7f}")
    for row in rows[1:]:
        lines.append(f"{row['name']}: {statistics.median(row['times']) / base:.3f} x the construct's time per step")
    lines.append(f"fit and step synchronised apart ({args.steps} steps per row): medians, and the peak rise of fit alone")
    lines.append(f"{'form':<26}{'fit ms':>16}{'step ms':>22}{'fit rise MB':>14}")
    for row in rows:
        lines.append(f"{row['name']:<26}{row['fit'] * 1e3:>16.3f}{row['opt_step'] * 1e3:>22.3f}{row['fit_rise'] / 1e6:>14.1f}")
    report = "\n".join(lines)
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
