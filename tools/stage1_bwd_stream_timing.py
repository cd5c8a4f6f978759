#!/usr/bin/env python3
"""The two forms of the stage-1 backward through the C ABI on the same operands, alternated:
  gemm    rtk_query_vectors_bwd_f32           W = dv . G^T and the Khatri-Rao operand written, two GEMMs
  stream  rtk_query_vectors_bwd_stream_f32    nothing of size B x a*b (rtk_query_bwd_stream.hip)
and, for bf16 operands, the gemm form on fp32 copies made per call (what the Python layer does on that route) against
rtk_query_vectors_bwd_stream_bf16 on the bf16 operands themselves.

Per shape: medians of --iters event-timed calls per round, --rounds rounds, and the peak of
torch.cuda.max_memory_allocated over the live bytes of one call (workspace, outputs and copies included).
  --iters N   --rounds N   --warmup N   --shapes B:a,b,c[:bf16] ..."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import r_tucker_amd as rt  # noqa: E402
from loss_stream_timing import peak_of, timed  # noqa: E402

DEFAULT = ["512:10,200,200", "2048:200,200,200", "8192:256,512,512", "8192:256,512,512:bf16"]
N_REL, N_SUB = 22, 40000


def one(spec, a):
    parts = spec.split(":")
    B, (ra, rb, rc), bf16 = int(parts[0]), (int(x) for x in parts[1].split(",")), len(parts) > 2 and parts[2] == "bf16"
    lib = rt._lib.load()
    g = torch.Generator(device="cuda").manual_seed(11)
    dt = torch.bfloat16 if bf16 else torch.float32
    core = (torch.randn((ra, rb, rc), device="cuda", generator=g) / np.sqrt(ra * rb)).to(dt)
    R = torch.randn((N_REL, ra), device="cuda", generator=g).to(dt)
    S = torch.randn((N_SUB, rb), device="cuda", generator=g).to(dt)
    dv = torch.randn((B, rc), device="cuda", generator=g) / B
    rel = torch.randint(0, N_REL, (B,), device="cuda", generator=g)
    sub = torch.randint(0, N_SUB, (B,), device="cuda", generator=g)
    sp = torch.cuda.current_stream().cuda_stream
    out = {}

    def call(form):
        def run():
            if form == "gemm":
                ops = [t.float() for t in (core, R, S)] if bf16 else [core, R, S]
                size, fn = lib.rtk_query_bwd_workspace_bytes, lib.rtk_query_vectors_bwd_f32
            else:
                ops = [core, R, S]
                size = lib.rtk_query_bwd_stream_workspace_bytes
                fn = lib.rtk_query_vectors_bwd_stream_bf16 if bf16 else lib.rtk_query_vectors_bwd_stream_f32
            gs = [torch.empty(t.shape, dtype=torch.float32, device="cuda") for t in (core, R, S)]
            ws = torch.empty(size(B, ra, rb, rc), dtype=torch.uint8, device="cuda")
            rt._lib.check(fn(ops[0].data_ptr(), ra, rb, rc, ops[1].data_ptr(), N_REL, ops[2].data_ptr(), N_SUB, rel.data_ptr(),
                             sub.data_ptr(), B, dv.data_ptr(), *[x.data_ptr() for x in gs], ws.data_ptr(), ws.numel(), sp), form)
            out[form] = gs
        return run

    forms = ("gemm", "stream")
    res = {f: [] for f in forms}
    for _ in range(a.rounds):                                  # alternated: gemm, stream, gemm, stream, ...
        for f in forms:
            res[f].append(timed(call(f), a.warmup, a.iters))
    peaks = {}
    for f in forms:
        out.clear()
        torch.cuda.empty_cache()
        peaks[f] = peak_of(call(f))
    gemm_ws = lib.rtk_query_bwd_workspace_bytes(B, ra, rb, rc) / 1e6
    stream_ws = lib.rtk_query_bwd_stream_workspace_bytes(B, ra, rb, rc) / 1e6
    print(f"== B {B}, rank ({ra}, {rb}, {rc}), {'bf16' if bf16 else 'fp32'} operands; workspace: gemm {gemm_ws:.1f} MB, "
          f"stream {stream_ws:.1f} MB")
    for f in forms:
        print(f"  {f:7}: " + "  ".join(f"{t:9.3f}" for t in res[f]) + f"  ms (median of {a.iters} per round); "
              f"peak over the live bytes {peaks[f]:9.1f} MB")
    m = {f: float(np.median(res[f])) for f in forms}
    print(f"  stream / gemm: time {m['stream'] / m['gemm']:.3f}, peak {peaks['stream'] / peaks['gemm']:.4f}")
    call("gemm")()
    ref = out["gemm"]
    call("stream")()
    torch.cuda.synchronize()
    for name, x, y in zip(("g_core", "g_R", "g_S"), out["stream"], ref):
        top = y.abs().max().item()
        print(f"  {name}: max|gemm| {top:.3e}, largest difference {(x - y).abs().max().item():.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", nargs="*", default=DEFAULT)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    for spec in a.shapes:
        one(spec, a)


if __name__ == "__main__":
    main()
