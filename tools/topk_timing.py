#!/usr/bin/env python3
"""Kernel times of the filtered top-k select (rtk_select_topk_*) next to the filtered-rank kernel that reads the same
row once; run under ``rocprofv3 --kernel-trace --stats`` for the per-kernel durations.

Shapes: WN18RR (B 512, N 40 943, fp32 scores of score_1vN with seeded parameters, WN18RR test queries and their
filter lists; k 10 and 1024) and one GPU's shard of the 1 M-entity configuration (B 8192, n 125 000, bf16 scores,
k 10).  Also prints wall-clock means (HIP events) of score_1vN, topk_1vN and the select alone at the WN18RR shape."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt                                   # noqa: E402
from r_tucker_amd.data import Data, KG_dataset              # noqa: E402

REPS = 20


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3      # us


data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
test_set = KG_dataset(data, data.test_data, test_set=True)
torch.manual_seed(1)
model = rt.AsymmetricR_TuckER((len(data.entities), len(data.relations)), (10, 200, 200))
model.init()
with torch.no_grad():
    model.core.mul_(3000.0)
model.cuda().eval()
flt = rt.DeviceFilter(test_set, "cuda")
items = torch.arange(512, device="cuda")
f = flt.features[items]
h, r, o = f[:, 0].contiguous(), f[:, 1].contiguous(), f[:, 2].contiguous()
core, R, S, O = model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data
with torch.no_grad():
    P = rt.score_1vN(core, R, S, O, h, r)
    res = {"filtered_rank (WN18RR)": timed(lambda: rt.filtered_ranks(P, o, flt, items))}
    for k in (10, 1024):
        res[f"select k={k} (WN18RR, filtered)"] = timed(lambda: rt.filtered_topk(P, k, flt, item_ids=items, keep_idx=o))
    res["score_1vN (WN18RR)"] = timed(lambda: rt.score_1vN(core, R, S, O, h, r))
    res["topk_1vN k=10 (WN18RR, filtered)"] = timed(lambda: rt.topk_1vN(core, R, S, O, h, r, 10, flt=flt))
    del P
    # one shard of the 1 M-entity configuration: bf16 scores (sigmoid of Gaussian logits), no filter
    g = torch.Generator(device="cuda").manual_seed(2)
    Pc = torch.sigmoid(torch.randn((8192, 125000), device="cuda", generator=g) * 3).to(torch.bfloat16)
    res["select k=10 (C5 shard, bf16)"] = timed(lambda: rt.filtered_topk(Pc, 10), reps=5)
torch.cuda.synchronize()
for name, us in res.items():
    print(f"{name:40s} {us:10.1f} us (wall clock, mean)")
