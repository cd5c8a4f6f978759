#!/usr/bin/env python3
"""Time rtk_tall_gram_f64 (csrc/rtk_tall_gram.hip; through smalllinalg.tall_gram_f64_rows, workspace allocation
included) against smalllinalg.tall_gram_f64 (the zero-padded float64 copy + batched rocBLAS product) on the Gram matrix
of an (n x k) fp32 block: the two alternate in one process after a warm-up, medians of event-timed calls, peak bytes of
each, and the kernel's FLOP/s.

usage: tools/tall_gram_timing.py [--calls 9] [--kernel-only] [n k ...]     (default shapes: 40943 200  125000 512)
--kernel-only runs just the kernel calls: the form to put behind `rocprofv3 --kernel-trace --stats --`, whose
per-kernel times are the kernel's own (an event pair around a call also holds the launch gaps and the allocator)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import r_tucker_amd as rt  # noqa: E402,F401
from r_tucker_amd import _lib, smalllinalg as sl  # noqa: E402

args = sys.argv[1:]
calls = 9
kernel_only = "--kernel-only" in args
args = [a for a in args if a != "--kernel-only"]
if "--calls" in args:
    i = args.index("--calls")
    calls = max(5, int(args[i + 1]))
    del args[i:i + 2]
shapes = [(int(args[i]), int(args[i + 1])) for i in range(0, len(args), 2)] or [(40943, 200), (125000, 512)]
lib = _lib.load()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


for n, k in shapes:
    D = torch.randn((n, k), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    kern, ref = (lambda: sl.tall_gram_f64_rows(D, D)), (lambda: sl.tall_gram_f64(D))
    if kernel_only:
        for _ in range(calls + 3):
            kern()
        torch.cuda.synchronize()
        continue
    for _ in range(3):
        kern(), ref()
    torch.cuda.synchronize()
    t_k, t_r = [], []
    for _ in range(calls):
        t_k.append(timed(kern)[0])
        t_r.append(timed(ref)[0])
    diff = (kern() - ref()).abs().max().item() / ref().abs().max().item()
    m_k, m_r = statistics.median(t_k), statistics.median(t_r)
    flop = 2.0 * n * k * k
    print(f"n {n} k {k}: kernel {m_k * 1e3:.0f} us (min {min(t_k) * 1e3:.0f}), torch float64 path {m_r * 1e3:.0f} us "
          f"(min {min(t_r) * 1e3:.0f}), medians of {calls}; kernel {flop / m_k / 1e9:.2f} TFLOP/s; "
          f"peak bytes kernel {peak(kern)} (workspace {lib.rtk_tall_gram_f64_workspace_bytes(n, k, k)}), "
          f"torch path {peak(ref)}; max |difference| / max |G| = {diff:.1e}")
