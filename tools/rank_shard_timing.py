#!/usr/bin/env python3
"""Per-batch times of filtered ranking on ONE rank's block of entity rows, two ways, in one process, alternated:

  (a) stored   the block path ShardedEntityScorer.filtered_ranks runs for a rank: score_1vN_into a (B, n_local) fp32
               block, target_scores_block, rank_counts_block;
  (c) blocks   the two matrix-free steps: stage 1 packed, ops.rank_targets_block, ops.rank_counts_block_1vN
               (count_kernel, entity-stationary).

(The former variant (b), ops.rank_1vN on the same rows as a problem of their own, ran a query-stationary kernel that no
longer exists: rank_1vN is now (c) at col0 = 0 in one library call; tools/rank_timing.py times it.)

Shapes: WN18RR (fp32, c 200, B 512, N 40 943 as one block, test queries with their filter lists; with and without
BCE), FB15k-237-like bf16 (c 200, B 2048, N 14 541) and one eighth of the 1 M-entity bf16 problem (c 512, B 8192,
n_local 125 000, col0 125 000, n_ent 1 000 000).  Prints wall-clock means per batch (HIP events); run under
``rocprofv3 --kernel-trace --stats`` for the per-kernel durations (profiles/rank_shard_kernel_stats.csv)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt                                   # noqa: E402
from r_tucker_amd.data import Data, KG_dataset              # noqa: E402
from r_tucker_amd.evaluation import rank_counts_block, target_scores_block   # noqa: E402


def alternate(variants, rounds=5, reps=4):
    """Mean microseconds per call of each variant; the variants take turns (rounds x reps calls each)."""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    tot = {k: 0.0 for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            tot[k] += a.elapsed_time(b)
    return {k: v / (rounds * reps) * 1e3 for k, v in tot.items()}


def shape(name, core, R, S, O_loc, col0, n_ent, h, r, t, flt, items, tables, want_bce, rounds=5, reps=4):
    B, n_loc = h.numel(), O_loc.shape[0]
    block = torch.empty((B, n_loc), dtype=torch.float32, device="cuda")
    slots = flt.slots_of(h, r) if flt is not None else None

    def stored():
        rt.score_1vN_into(core, R, S, O_loc, h, r, out=block, tables=tables)
        pt = target_scores_block(block, t, col0)
        return rank_counts_block(block, t, col0, pt, flt, items, want_bce)

    def blocks():
        _, qp = rt.query_vectors(core, R, S, h, r, tables=tables, packed=True)
        pt = rt.rank_targets_block(qp, B, O_loc, col0, n_ent, t)
        return rt.rank_counts_block_1vN(qp, B, O_loc, col0, n_ent, pt, t, flt=flt, slots=slots, want_bce=want_bce)

    us = alternate({"stored": stored, "blocks": blocks}, rounds, reps)
    print(f"{name:44s} (a) stored {us['stored']:10.1f}  (c) blocks {us['blocks']:10.1f} us (wall clock per batch)")


with rt.index_check("off"), torch.no_grad():
    data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
    test_set = KG_dataset(data, data.test_data, test_set=True)
    torch.manual_seed(1)
    model = rt.AsymmetricR_TuckER((len(data.entities), len(data.relations)), (10, 200, 200))
    model.init()
    model.core.mul_(3000.0)
    model.cuda().eval()
    flt = rt.DeviceFilter(test_set, "cuda")
    items = torch.arange(512, device="cuda")
    f = flt.features[items]
    h, r, o = f[:, 0].contiguous(), f[:, 1].contiguous(), f[:, 2].contiguous()
    core, R, S, O = model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data.contiguous()
    tables = rt.relation_tables(core, R)
    N = O.shape[0]
    shape("WN18RR fp32 c 200 B 512, filter", core, R, S, O, 0, N, h, r, o, flt, items, tables, False)
    shape("WN18RR fp32 c 200 B 512, filter + BCE", core, R, S, O, 0, N, h, r, o, flt, items, tables, True)

    g = torch.Generator(device="cuda").manual_seed(2)
    N, c, B = 14541, 200, 2048
    coreb = (torch.randn((10, c, c), device="cuda", generator=g) * (3.0 / (10 * c * c) ** 0.5)).to(torch.bfloat16)
    Rb = torch.randn((237, 10), device="cuda", generator=g).to(torch.bfloat16)
    Eb = torch.randn((N, c), device="cuda", generator=g).to(torch.bfloat16)
    hb, rb, tb = (torch.randint(0, N, (B,), device="cuda", generator=g), torch.randint(0, 237, (B,), device="cuda", generator=g),
                  torch.randint(0, N, (B,), device="cuda", generator=g))
    tab = rt.relation_tables(coreb, Rb)
    shape("bf16 c 200 B 2048 N 14 541", coreb, Rb, Eb, Eb, 0, N, hb, rb, tb, None, None, tab, False)
    del Eb

    n_ent, n_loc, col0, c, B = 1_000_000, 125_000, 125_000, 512, 8192
    coreb = (torch.randn((4, c, c), device="cuda", generator=g) * (3.0 / (4 * c * c) ** 0.5)).to(torch.bfloat16)
    Rb = torch.randn((11, 4), device="cuda", generator=g).to(torch.bfloat16)
    Sb = (torch.randn((n_loc, c), device="cuda", generator=g) / c ** 0.5 * 4).to(torch.bfloat16)   # subject rows in use
    Ob = (torch.randn((n_loc, c), device="cuda", generator=g) / c ** 0.5 * 4).to(torch.bfloat16)   # the rank's rows of O
    hb, rb, tb = (torch.randint(0, n_loc, (B,), device="cuda", generator=g), torch.randint(0, 11, (B,), device="cuda", generator=g),
                  torch.randint(0, n_ent, (B,), device="cuda", generator=g))
    tab = rt.relation_tables(coreb, Rb)
    shape("1 M / 8 shard bf16 c 512 B 8192 n_local 125 000", coreb, Rb, Sb, Ob, col0, n_ent, hb, rb, tb, None, None, tab,
          False, rounds=3, reps=2)
torch.cuda.synchronize()
