#!/usr/bin/env python3
"""Kernel times of candidate scoring (rtk_score_candidates_*: forward, dv backward, dO backward); run under
``rocprofv3 --kernel-trace --stats`` for the per-kernel durations.

Points: the WN18RR shape (fp32, c 200, N 40 943, B 512, K 1 / 16 / 128 / 1024), the 1 M-entity bf16 problem (c 512,
N 1 000 000, B 8192, K 256, uniformly random per-query lists) and B 65 536 triples (K 1, WN18RR table).  For each the
effective gather rate  B K (c s + 12) + B c 4  bytes over the forward's wall-clock time (HIP events, mean), and, next to
it, score_1vN plus a torch.gather of the same entries."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt                                   # noqa: E402

lib = rt._lib.load()


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


def point(name, N, c, B, K, dtype, n_rel=11, a=10, with_1vN=True, reps=20):
    g = torch.Generator(device="cuda").manual_seed(B + K)
    core = (torch.randn((a, c, c), device="cuda", generator=g) * (3.0 / (a * c * c) ** 0.5)).to(dtype)
    R = torch.randn((n_rel, a), device="cuda", generator=g).to(dtype)
    S = torch.randn((N, c), device="cuda", generator=g).to(dtype)
    O = torch.randn((N, c), device="cuda", generator=g).to(dtype)
    h = torch.randint(0, N, (B,), device="cuda", generator=g)
    r = torch.randint(0, n_rel, (B,), device="cuda", generator=g)
    cand = torch.randint(0, N, (B, K), device="cuda", generator=g)
    v = rt.query_vectors(core, R, S, h, r)
    bf16 = dtype == torch.bfloat16
    sfx = "_bf16" if bf16 else "_f32"
    out = torch.empty((B, K), dtype=torch.float32, device="cuda")
    dz = torch.randn((B, K), device="cuda", generator=g)
    dv = torch.empty((B, c), dtype=torch.float32, device="cuda")
    gO = torch.empty((N, c), dtype=torch.float32, device="cuda")
    ws = torch.zeros(max(lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N), 256), dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    fwd_fn, bwd_fn = getattr(lib, "rtk_score_candidates" + sfx), getattr(lib, "rtk_score_candidates_bwd" + sfx)
    flags = rt._lib.RTK_SCORE_SIGMOID | rt._lib.RTK_SCORE_SIGMOID_FAST

    def fwd():
        rt._lib.check(fwd_fn(v.data_ptr(), B, c, O.data_ptr(), N, cand.data_ptr(), K, K, out.data_ptr(), K, flags,
                             ws.data_ptr(), ws.numel(), sp), "fwd")

    def bwd_dv():
        rt._lib.check(bwd_fn(dz.data_ptr(), K, v.data_ptr(), B, c, O.data_ptr(), N, cand.data_ptr(), K, K, dv.data_ptr(),
                             None, ws.data_ptr(), ws.numel(), sp), "dv")

    def bwd_do():
        rt._lib.check(bwd_fn(dz.data_ptr(), K, v.data_ptr(), B, c, O.data_ptr(), N, cand.data_ptr(), K, K, None,
                             gO.data_ptr(), ws.data_ptr(), ws.numel(), sp), "dO")

    s = O.element_size()
    nbytes = B * K * (c * s + 12) + B * c * 4
    t = {"fwd": timed(fwd, reps), "dv": timed(bwd_dv, reps), "dO": timed(bwd_do, reps)}
    line = (f"{name:34s} fwd {t['fwd']:9.1f} us  {nbytes / t['fwd'] / 1e6:6.2f} TB/s ({nbytes / 1e6:8.1f} MB)"
            f"  dv {t['dv']:9.1f} us ({t['dv'] / t['fwd']:4.2f}x)  dO {t['dO']:9.1f} us ({t['dO'] / t['fwd']:4.2f}x)")
    if with_1vN:
        with torch.no_grad():
            t1 = timed(lambda: rt.score_1vN(core, R, S, O, h, r).gather(1, cand), reps=max(3, reps // 4))
        line += f"  | score_1vN + gather {t1:9.1f} us"
    print(line, flush=True)
    del core, R, S, O, gO, ws
    torch.cuda.empty_cache()


with torch.no_grad():
    for K in (1, 16, 128, 1024):
        point(f"WN18RR fp32 c200 B512 K{K}", 40943, 200, 512, K, torch.float32)
    point("triples fp32 c200 B65536 K1", 40943, 200, 65536, 1, torch.float32)
    point("1M bf16 c512 B8192 K256", 1_000_000, 512, 8192, 256, torch.bfloat16, a=16, reps=10)
