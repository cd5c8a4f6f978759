#!/usr/bin/env python3
"""Forward + backward of bce_loss_1vN in its two forms (the (B, N) matrix written and re-read / matrix_free=True),
event-timed, with torch.cuda.max_memory_allocated, at the WN18RR shape (N 40 943, rank (10, 200, 200), B 512) and at
N = 1 000 000, rank (10, 200, 200), B 4096; at the second shape also rank_counts_block_1vN(..., want_bce=True) over the
whole matrix as one block: count_kernel with BCE is the same sweep without the second tile product.  The forms are
alternated in one process.  Kernel medians: run under `rocprofv3 --kernel-trace --stats -- python tools/loss_stream_timing.py`.
  --shape wn18rr | big | both      --iters N"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gen  # noqa: E402
import r_tucker_amd as rt  # noqa: E402


class SyntheticPairs:
    """The attributes DeviceFilter reads from a KG_dataset: n_pairs (subject, relation) pairs with 1..8 known objects."""

    def __init__(self, n_ent, n_rel, n_pairs, seed):
        rng = np.random.default_rng(seed)
        self._pairs = np.stack([rng.permutation(n_ent)[:n_pairs], rng.integers(0, n_rel, n_pairs)], 1).astype(np.int64)
        lens = rng.integers(1, 9, n_pairs)
        self._ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self._obj = rng.integers(0, n_ent, int(lens.sum())).astype(np.int64)
        self.features = self._pairs


def timed(fn, warm, iters):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def run(name, n_ent, n_rel, rank, B, flt, ids, warm, iters, yardstick):
    core, R, S, O = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gen.make_params(n_ent, n_rel, rank, 322)]
    f = flt.features[ids]
    h, r = f[:, 0].contiguous(), f[:, 1].contiguous()

    def step(matrix_free):
        for p in (core, R, S, O):
            p.grad = None
        loss = rt.bce_loss_1vN(core, R, S, O, h, r, flt, ids, label_smoothing=0.1, matrix_free=matrix_free)
        loss.backward()
        return loss

    def fwd(matrix_free):
        with torch.no_grad():
            return rt.bce_loss_1vN(core, R, S, O, h, r, flt, ids, label_smoothing=0.1, matrix_free=matrix_free)

    print(f"== {name}: N {n_ent}, rank {rank}, B {B}; the matrix is {B * n_ent * 4 / 1e6:.0f} MB")
    res = {}
    for _ in range(2):                                       # alternated: matrix, matrix-free, matrix, matrix-free
        for mf in (False, True):
            res.setdefault(mf, []).append((timed(lambda: step(mf), warm, iters), timed(lambda: fwd(mf), warm, iters)))
    for mf in (False, True):
        t_step = min(x[0] for x in res[mf])
        t_fwd = min(x[1] for x in res[mf])
        print(f"  matrix_free={mf!s:5}: forward+backward {t_step:9.3f} ms  loss-only forward {t_fwd:9.3f} ms  "
              f"peak over the live bytes {peak_of(lambda: step(mf)):9.1f} MB  loss {step(mf).item():.6f}")
    if yardstick:
        with torch.no_grad():
            v, qp = rt.query_vectors(core, R, S, h, r, packed=True)
            t = f[:, 0].contiguous()                         # any valid object ids
            pt = rt.rank_targets_block(qp, B, O.detach(), 0, n_ent, t)
            slots = flt.slots_of(h, r)
            ms = timed(lambda: rt.rank_counts_block_1vN(qp, B, O.detach(), 0, n_ent, pt, t, flt=flt, slots=slots,
                                                        want_bce=True), warm, iters)
        print(f"  rank_counts_block_1vN(want_bce=True), one block: {ms:9.3f} ms")


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
            torch.arange(2000, 2000 + 512).cuda(), a.warmup, a.iters, False)
    if a.shape in ("big", "both"):
        n_ent, n_rel, B = 1_000_000, 22, 4096
        flt = rt.DeviceFilter(SyntheticPairs(n_ent, n_rel, B, 1), "cuda")
        run("1 M entities", n_ent, n_rel, (10, 200, 200), B, flt, torch.arange(B).cuda(), a.warmup, a.iters, True)
