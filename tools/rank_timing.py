#!/usr/bin/env python3
"""Kernel times of filtered ranking without the score matrix (ops.rank_1vN: target_kernel, count_kernel,
filter_kernel, finish_kernel) and of the tie counts (ops.rank_ties_1vN: the same kernels in their tie form)
next to the stored path it replaces (score_1vN + filtered_ranks); run under ``rocprofv3 --kernel-trace --stats`` for the
per-kernel durations.

Shapes: WN18RR (B 512, N 40 943, c 200, fp32, relation tables cached, WN18RR test queries and their filter lists),
FB15k-237-like bf16 (B 2048, N 14 541, c 200, symmetric) and the 1 M-entity bf16 problem (B 8192, c 512).  Also prints
wall-clock means (HIP events) per call."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt                                   # noqa: E402
from r_tucker_amd.data import Data, KG_dataset              # noqa: E402


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3      # us


res = {}
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
    core, R, S, O = model.core.data, model.R.weight.data, model.S.weight.data, model.O.weight.data
    tables = rt.relation_tables(core, R)
    res["rank_1vN (WN18RR, tables)"] = timed(lambda: rt.rank_1vN(core, R, S, O, h, r, o, flt=flt, tables=tables))
    res["rank_1vN +bce (WN18RR, tables)"] = timed(
        lambda: rt.rank_1vN(core, R, S, O, h, r, o, flt=flt, want_bce=True, tables=tables))
    res["rank_ties_1vN (WN18RR, tables)"] = timed(lambda: rt.rank_ties_1vN(core, R, S, O, h, r, o, flt=flt, tables=tables))
    res["score_1vN + filtered_ranks (WN18RR, tables)"] = timed(
        lambda: rt.filtered_ranks(rt.score_1vN(core, R, S, O, h, r, tables=tables), o, flt, items))

    g = torch.Generator(device="cuda").manual_seed(2)
    N, c, B = 14541, 200, 2048
    coreb = (torch.randn((10, c, c), device="cuda", generator=g) * (3.0 / (10 * c * c) ** 0.5)).to(torch.bfloat16)
    Rb = torch.randn((237, 10), device="cuda", generator=g).to(torch.bfloat16)
    Eb = torch.randn((N, c), device="cuda", generator=g).to(torch.bfloat16)
    hb, rb, tb = (torch.randint(0, N, (B,), device="cuda", generator=g), torch.randint(0, 237, (B,), device="cuda", generator=g),
                  torch.randint(0, N, (B,), device="cuda", generator=g))
    tab = rt.relation_tables(coreb, Rb)
    res["rank_1vN (FB15k-237-like bf16, B 2048)"] = timed(lambda: rt.rank_1vN(coreb, Rb, Eb, Eb, hb, rb, tb, tables=tab))
    res["rank_ties_1vN (FB15k-237-like bf16, B 2048)"] = timed(lambda: rt.rank_ties_1vN(coreb, Rb, Eb, Eb, hb, rb, tb, tables=tab))
    res["score_1vN + filtered_ranks (bf16, B 2048)"] = timed(
        lambda: rt.filtered_ranks(rt.score_1vN(coreb, Rb, Eb, Eb, hb, rb, tables=tab), tb))
    del Eb

    N, c, B = 1_000_000, 512, 8192
    coreb = (torch.randn((4, c, c), device="cuda", generator=g) * (3.0 / (4 * c * c) ** 0.5)).to(torch.bfloat16)
    Rb = torch.randn((11, 4), device="cuda", generator=g).to(torch.bfloat16)
    Eb = (torch.randn((N, c), device="cuda", generator=g) / c ** 0.5 * 4).to(torch.bfloat16)
    hb, rb, tb = (torch.randint(0, N, (B,), device="cuda", generator=g), torch.randint(0, 11, (B,), device="cuda", generator=g),
                  torch.randint(0, N, (B,), device="cuda", generator=g))
    tab = rt.relation_tables(coreb, Rb)
    res["rank_1vN (1M bf16, c 512, B 8192)"] = timed(lambda: rt.rank_1vN(coreb, Rb, Eb, Eb, hb, rb, tb, tables=tab),
                                                     reps=2)
torch.cuda.synchronize()
for name, us in res.items():
    print(f"{name:48s} {us:12.1f} us (wall clock, mean)")
for shape in ("(WN18RR, tables)", "(FB15k-237-like bf16, B 2048)"):
    print(f"rank_ties_1vN / rank_1vN {shape}: {res['rank_ties_1vN ' + shape] / res['rank_1vN ' + shape]:.3f}")
