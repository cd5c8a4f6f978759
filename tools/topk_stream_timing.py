#!/usr/bin/env python3
"""Filtered top-k in its three forms -- (a) topk_1vN default (the (B, N) scores in a buffer), (b) entity_block=250 000
(where N is larger than one block), (c) matrix_free=True -- event-timed per call, with torch.cuda.max_memory_allocated
over the live bytes, rtk_score_topk_workspace_bytes next to it, and the share of (c) spent in the entity-stationary
sweep (tmax_kernel, from the library's kernel timer; the rest is the filter patch, the two selects and the gather).
The forms are alternated in one process and checked against each other where their scores have the same bits.

  wn18rr   fp32, N 40 943, rank (10, 200, 200), B 512, k 10, the train split's filter
  shard    bf16, one 125 000-row shard of 1 000 000 entities, c 512, B 8192, k 10
  big      fp32, N 1 000 000, rank (10, 200, 200), B 4096, k 10

Without --shape every shape runs in a child process of its own under a time limit; the first failure ends the run.
  --shape wn18rr | shard | big     --iters N  --warmup N  --limit SECONDS  --out FILE"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
SHAPES = ("wn18rr", "shard", "big")
BLOCK = 250_000


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


def sweep_ms(rt, fn, iters):
    """median time of the first score-kernel launch of fn (the sweep), from the kernel's own begin / end stamps"""
    lib = rt._lib.load()
    h = C.c_void_p()
    rt._lib.check(lib.rtk_timer_create(C.byref(h)), "rtk_timer_create")
    ts = []
    for _ in range(iters):
        rt._lib.check(lib.rtk_timer_arm(h), "rtk_timer_arm")
        fn()
        torch.cuda.synchronize()
        ms = C.c_float()
        rt._lib.check(lib.rtk_timer_elapsed_ms(h, C.byref(ms)), "rtk_timer_elapsed_ms")
        ts.append(ms.value)
    lib.rtk_timer_destroy(h)
    return float(np.median(ts))


def params(n_ent, n_rel, rank, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a, b, c = rank
    core = torch.randn(a, b, c, device="cuda", generator=g) / (b * a) ** 0.5
    R = torch.randn(n_rel, a, device="cuda", generator=g)
    S = torch.randn(n_ent, b, device="cuda", generator=g) / b ** 0.5
    O = torch.randn(n_ent, c, device="cuda", generator=g) * 3.0
    return [t.to(dtype) for t in (core, R, S, O)]


def run(name, a):
    import r_tucker_amd as rt
    k = 10
    if name == "wn18rr":
        import gen
        from r_tucker_amd.data import Data, KG_dataset
        data = Data(os.path.join(ROOT, "data", "WN18RR") + "/", reverse=True)
        flt = rt.DeviceFilter(KG_dataset(data, data.train_data), "cuda")
        n_ent, n_rel, rank, B, dtype = len(data.entities), len(data.relations), (10, 200, 200), 512, torch.float32
        core, R, S, O = [torch.from_numpy(x).cuda() for x in gen.make_params(n_ent, n_rel, rank, 322, logit_std=3.0)]
        col0, n_all = 0, n_ent
    elif name == "shard":
        n_all, n_ent, n_rel, rank, B, dtype = 1_000_000, 125_000, 22, (10, 512, 512), 8192, torch.bfloat16
        flt = rt.DeviceFilter(SyntheticPairs(n_all, n_rel, B, 1), "cuda")
        core, R, S, O = params(n_ent, n_rel, rank, dtype, 2)
        col0 = 3 * n_ent                                         # the fourth of eight shards
    else:
        n_all = n_ent = 1_000_000
        n_rel, rank, B, dtype, col0 = 22, (10, 200, 200), 4096, torch.float32, 0
        flt = rt.DeviceFilter(SyntheticPairs(n_all, n_rel, B, 1), "cuda")
        core, R, S, O = params(n_ent, n_rel, rank, dtype, 3)
    f = flt.features[:B]
    h, r = f[:, 0].contiguous() % S.shape[0], f[:, 1].contiguous()
    slots = flt.slots_of(f[:, 0].contiguous(), r)
    fx = type("F", (), {"pair_ptr": flt.pair_ptr, "pair_obj": flt.pair_obj, "slots_of": staticmethod(lambda hh, rr: slots)})
    dcode = 1 if dtype == torch.bfloat16 else 0
    ws = rt._lib.load().rtk_score_topk_workspace_bytes(dcode, min(B, rt.ops._topk_stream_chunk(dcode, B, n_ent, rank[2], k)),
                                                       n_ent, rank[2], k)
    print(f"== {name}: {str(dtype)[6:]}, rows {n_ent} of {n_all}, rank {rank}, B {B}, k {k}; the score block is "
          f"{B * n_ent * 4 / 1e6:.0f} MB, rtk_score_topk_workspace_bytes {ws / 1e6:.1f} MB", flush=True)
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    forms = {}
    if col0 == 0:
        forms["(a) default"] = lambda: rt.topk_1vN(core, R, S, O, h, r, k, flt=fx)
        if n_ent > BLOCK:
            forms[f"(b) entity_block={BLOCK}"] = lambda: rt.topk_1vN(core, R, S, O, h, r, k, flt=fx, entity_block=BLOCK)
        forms["(c) matrix_free"] = lambda: rt.topk_1vN(core, R, S, O, h, r, k, flt=fx, matrix_free=True)
    else:
        buf = torch.empty((B, n_ent), dtype=torch.float32, device="cuda")

        def stored():
            rt.score_packed_into(qp, B, O, buf)
            return rt.filtered_topk(buf, k, fx, slots=slots, col0=col0)
        forms["(a) score block + select (stage 2 only)"] = stored
        forms["(c) topk_block_1vN (stage 2 only)"] = lambda: rt.topk_block_1vN(qp, B, O, col0, n_all, k, flt=fx, slots=slots)
    res = {n_: [] for n_ in forms}
    for _ in range(2):                                           # alternated
        for n_, fn in forms.items():
            res[n_].append(timed(fn, a.warmup, a.iters))
    out = {}
    for n_, fn in forms.items():
        out[n_] = fn()
        extra = ""
        if n_.startswith("(c)"):
            extra = f"  sweep kernel {sweep_ms(rt, fn, a.iters):9.3f} ms"
        print(f"  {n_:42}: {min(res[n_]):9.3f} ms per call  peak over the live bytes {peak_of(fn):9.1f} MB{extra}", flush=True)
    names = list(out)
    same = [bool(torch.equal(out[names[0]][1], out[n_][1])) for n_ in names[1:]]
    agree = [float((out[names[0]][1] == out[n_][1]).float().mean()) for n_ in names[1:]]
    print(f"  ids equal to {names[0]}'s: {dict(zip(names[1:], same))} (share of equal entries {agree}; the default fp32 "
          "kernel differs from the ws kernel's bits on its fifth-group columns only)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=SHAPES)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape (child process)")
    ap.add_argument("--out", help="also append the output to this file")
    a = ap.parse_args()
    if a.shape:
        run(a.shape, a)
        sys.exit(0)
    for s in SHAPES:                                             # one child per shape, each under its own limit
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--shape", s,
               "--iters", str(a.iters), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(p.stdout, end="", flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(p.stdout)
        if p.returncode != 0:
            print(f"{s}: exit status {p.returncode}; stopping", flush=True)
            sys.exit(p.returncode)
