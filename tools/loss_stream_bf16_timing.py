#!/usr/bin/env python3
"""One C5 shard on one GPU: the 1-vs-all BCE loss on 125 000 bf16 entity rows of a 1 000 000-entity matrix at rank
(256, 512, 512), B 8192 -- the matrix-free block form (bce_loss_block_1vN over rtk_bce_stream_*_part_bf16) against the
matrix form (bce_loss_1vN(matrix_free=False)) on the same bf16 operands, alternated.

The matrix form has no block variant, so it runs on a 125 000-entity matrix holding the shard's rows: the same dense
work (B x 125 000 scores, the two B x N sized GEMMs), with its own smoothing term and only the positives that fall
into [0, 125 000) -- the loss values differ, the work does not.  The block form runs as the first shard (col0 = 0,
n_ent = 1 000 000), so both own the same CSR entries.

Recorded: forward + backward, the loss-only forward (torch.no_grad), and the peak of torch.cuda.max_memory_allocated
over the live bytes, per form; medians of --iters event-timed calls per round, --rounds rounds.
  --iters N   --rounds N   --warmup N   --batch B   --rank a,b,c   --rows n_local"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import r_tucker_amd as rt  # noqa: E402
from r_tucker_amd.synthetic import make_params  # noqa: E402
from loss_stream_timing import SyntheticPairs, peak_of, timed  # noqa: E402

N_ENT, N_REL, EPS = 1_000_000, 22, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--rank", default="256,512,512")
    ap.add_argument("--rows", type=int, default=125_000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    rank, B, n_loc = tuple(int(x) for x in a.rank.split(",")), a.batch, a.rows
    # the parameters of the shard only: subjects and objects among its rows
    core, R, S, O = make_params(n_loc, N_REL, rank, 322)
    core, R, S, O = [torch.from_numpy(x).cuda().bfloat16().requires_grad_(True) for x in (core, R, S, O)]
    flt = rt.DeviceFilter(SyntheticPairs(n_loc, N_REL, B, 1), "cuda")
    ids = torch.arange(B).cuda()
    f = flt.features[ids]
    h, r = f[:, 0].contiguous(), f[:, 1].contiguous()

    def block():
        return rt.bce_loss_block_1vN(core, R, S, O, 0, N_ENT, h, r, flt, ids, label_smoothing=EPS)

    def matrix():
        return rt.bce_loss_1vN(core, R, S, O, h, r, flt, ids, label_smoothing=EPS)

    def step(loss_fn):
        def run():
            for p in (core, R, S, O):
                p.grad = None
            loss = loss_fn()
            loss.backward()
            return loss
        return run

    def forward(loss_fn):
        def run():
            with torch.no_grad():
                return loss_fn()
        return run

    forms = (("matrix form (n_ent = the shard's rows)", matrix), ("block form, matrix-free", block))
    print(f"== one C5 shard: {n_loc} bf16 rows, rank {rank}, B {B}; the (B, n_local) fp32 matrix is "
          f"{B * n_loc * 4 / 1e6:.0f} MB, the fp32 copy of O_loc {n_loc * rank[2] * 4 / 1e6:.0f} MB")
    res = {}
    for _ in range(a.rounds):                                     # alternated: matrix, block, matrix, block, ...
        for name, fn in forms:
            res.setdefault((name, "forward + backward"), []).append(timed(step(fn), a.warmup, a.iters))
            res.setdefault((name, "loss-only forward"), []).append(timed(forward(fn), a.warmup, a.iters))
    for name, fn in forms:
        for p in (core, R, S, O):
            p.grad = None
        pk_step, pk_fwd = peak_of(step(fn)), peak_of(forward(fn))
        for what, pk in (("forward + backward", pk_step), ("loss-only forward", pk_fwd)):
            ts = res[(name, what)]
            print(f"  {name:40} {what:18}: " + "  ".join(f"{t:9.3f}" for t in ts) + f"  ms (median of {a.iters} per round); "
                  f"peak over the live bytes {pk:9.1f} MB")
    for what in ("forward + backward", "loss-only forward"):
        m, b = (float(np.median(res[(name, what)])) for name, _ in forms)
        print(f"  {what}: block / matrix = {b / m:.3f}")
    print(f"  loss: matrix form (its own n_ent) {matrix().item():.6f}; the block's share {block().item():.6f}")


if __name__ == "__main__":
    main()
