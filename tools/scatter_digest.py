#!/usr/bin/env python3
"""SHA-256 of every output that passes through the ordered scatter (csrc/rtk_scatter.hip), on fixed seeds, through the
C entries: gO and dv of rtk_score_candidates_bwd_{f32,bf16} on both sides of 65 536 entries (windows of 16 and of 32),
gO of rtk_bce_stream_grad_o_f32 and of its _part form on two blocks, dv and gO of rtk_ce_stream_grad_f32, the stream
entries at two values of max_pos on opposite sides of 65 536 with one CSR list of 300 entries (longer than the flat
window of 256).  One line per output; two builds of the library compute the same thing when the lines are equal:

    R_TUCKER_AMD_LIB=/path/to/other/librtucker_hip.so python tools/scatter_digest.py > a.txt
    python tools/scatter_digest.py > b.txt && diff a.txt b.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import r_tucker_amd as rt  # noqa: E402

SIGMOID = 1


def stream():
    return torch.cuda.current_stream().cuda_stream


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def report(name, t):
    print(f"{name:44s} {sha(t)}", flush=True)


def ok(lib, rc):
    assert rc == 0, lib.rtk_last_error_string()


def randn(g, *shape, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).cuda()


def candidates(lib):
    N, B, c = 5000, 1100, 40
    for K in (32, 64):                                           # M = 35 200 and 70 400
        g = torch.Generator().manual_seed(100 + K)
        v, O, dz = randn(g, B, c), randn(g, N, c), randn(g, B, K)
        cand = torch.randint(0, N, (B, K), generator=g)
        cand[:, 5] = 7                                           # one entity in every row: a run of B entries
        cand[3, 9], cand[4, 9] = -1, N                           # invalid ids add nothing
        cand = cand.cuda()
        nws = lib.rtk_score_candidates_bwd_workspace_bytes(B, K, N)
        for name, fn, Od in (("f32", lib.rtk_score_candidates_bwd_f32, O), ("bf16", lib.rtk_score_candidates_bwd_bf16, O.bfloat16())):
            ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
            dv = torch.full((B, c), float("nan"), device="cuda")
            gO = torch.full((N, c), float("nan"), device="cuda")
            ok(lib, fn(dz.data_ptr(), K, v.data_ptr(), B, c, Od.data_ptr(), N, cand.data_ptr(), K, K, dv.data_ptr(),
                       gO.data_ptr(), ws.data_ptr(), nws, stream()))
            report(f"score_candidates_bwd_{name} M={B * K} gO", gO)
            report(f"score_candidates_bwd_{name} M={B * K} dv", dv)


def losses(lib):
    N, B, c, eps = 3000, 512, 64, 0.1
    g = torch.Generator().manual_seed(7)
    v, O = randn(g, B, c, scale=0.3), randn(g, N, c, scale=0.3)
    lens = torch.randint(1, 60, (B,), generator=g)
    lens[17] = 300                                               # longer than the flat window
    lens[40] = 0
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    entries = int(ptr[-1])
    obj = torch.randint(0, N, (entries,), generator=g)
    obj[::50] = 11                                               # a long run of one entity
    slot = torch.randperm(B, generator=g)
    slot[5] = -1                                                 # a query without a list
    slot, ptr, obj = slot.cuda(), ptr.cuda(), obj.cuda()
    csr = (slot.data_ptr(), ptr.data_ptr(), obj.data_ptr())
    scale = torch.tensor([1.0 / B], device="cuda")
    qp = torch.empty(lib.rtk_packed_query_bytes(0, B, c), dtype=torch.uint8, device="cuda")
    ok(lib, lib.rtk_pack_query_vectors(v.data_ptr(), B, c, 0, qp.data_ptr(), stream()))
    assert entries < 65536
    # the forward of the cross-entropy gives lse
    nws = lib.rtk_ce_stream_workspace_bytes(B, N, c, 0)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    rows, lse = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, device="cuda")
    ok(lib, lib.rtk_ce_stream_rows_f32(qp.data_ptr(), B, c, O.data_ptr(), N, *csr, eps, rows.data_ptr(), lse.data_ptr(),
                                       ws.data_ptr(), nws, stream()))
    for max_pos in (entries, 70000):
        tag = f"max_pos={max_pos}"
        nws = lib.rtk_bce_stream_workspace_bytes(B, N, c, max_pos)
        ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
        gO = torch.full((N, c), float("nan"), device="cuda")
        ok(lib, lib.rtk_bce_stream_grad_o_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), N, *csr, max_pos, eps, SIGMOID,
                                              scale.data_ptr(), gO.data_ptr(), ws.data_ptr(), nws, stream()))
        report(f"bce_stream_grad_o_f32 {tag} gO", gO)
        gP = torch.full((N, c), float("nan"), device="cuda")
        for col0, n_local in ((0, 1300), (1300, N - 1300)):
            nws = lib.rtk_bce_stream_part_workspace_bytes(B, n_local, c, max_pos)
            ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
            ok(lib, lib.rtk_bce_stream_grad_o_part_f32(qp.data_ptr(), v.data_ptr(), B, c, O[col0:].data_ptr(), n_local, col0, N,
                                                       *csr, max_pos, eps, SIGMOID, scale.data_ptr(), gP[col0:].data_ptr(),
                                                       ws.data_ptr(), nws, stream()))
        report(f"bce_stream_grad_o_part_f32 {tag} gO", gP)
        nws = lib.rtk_ce_stream_workspace_bytes(B, N, c, max_pos)
        ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
        dv = torch.full((B, c), float("nan"), device="cuda")
        gO = torch.full((N, c), float("nan"), device="cuda")
        ok(lib, lib.rtk_ce_stream_grad_f32(qp.data_ptr(), v.data_ptr(), B, c, O.data_ptr(), N, *csr, max_pos, eps,
                                           lse.data_ptr(), scale.data_ptr(), dv.data_ptr(), gO.data_ptr(), ws.data_ptr(), nws,
                                           stream()))
        report(f"ce_stream_grad_f32 {tag} dv", dv)
        report(f"ce_stream_grad_f32 {tag} gO", gO)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    lib = rt._lib.load()
    print(f"# {os.path.relpath(rt._lib.LIB_PATH, ROOT)}", file=sys.stderr)
    candidates(lib)
    losses(lib)
