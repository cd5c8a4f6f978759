#!/usr/bin/env python3
"""One rank of P = 8 on one GPU (no collective): the matrix-free training loss on a block of 125 000 rows of a
1 000 000-entity matrix (B 4096, rank (10, 200, 200), fp32, fast logistic).

  abi   the two block entry points (rtk_bce_stream_rows_part_f32 / rtk_bce_stream_grad_o_part_f32, col0 = 375 000,
        n_ent = 1 000 000) against the whole-matrix entry points on a 125 000-entity matrix holding the same rows
        (the CSR ids shifted by col0, so the entries of the other blocks fall outside [0, 125 000) and are skipped):
        the same dense work; the block form adds the ownership test and the padding of the flat lists.  Alternated,
        medians of --iters event-timed calls per round, --rounds rounds; the yardstick's spread over its own rounds is
        the margin.  --yardstick-lib PATH takes the whole-matrix entry points from another build of the library
        (the parent commit's); default: this build's.  With eps = 0 the two forms must give the same bits (checked).
  step  forward + backward of bce_loss_block_1vN on the block against bce_loss_1vN(matrix_free=True) on the whole
        1 M-entity matrix, with the peak of torch.cuda.max_memory_allocated over the live bytes.

  --loss ce   the softmax cross-entropy loss instead (the step part only): forward + backward of
        ce_loss_block_1vN(..., lse=) on the block -- what one rank of 8 computes, the three exchanges left out; the
        global lse comes once, untimed, from ce_partials_block_1vN on all eight blocks and ce_merge_lse -- against
        ce_loss_1vN(matrix_free=True) on the whole 1 M-entity matrix, alternated, with the peaks.

Kernel medians: `rocprofv3 --kernel-trace --stats -- python tools/loss_shard_timing.py --part abi`.
  --part abi | step | both    --loss bce | ce    --iters N    --rounds N    --yardstick-lib PATH"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import gen  # noqa: E402
import r_tucker_amd as rt  # noqa: E402
from loss_stream_timing import SyntheticPairs, peak_of, timed  # noqa: E402

N_ENT, N_REL, B, RANK, P_RANKS, BLOCK = 1_000_000, 22, 4096, (10, 200, 200), 8, 3
EPS = 0.1


def whole_entry_points(path):
    """rtk_bce_stream_rows_f32 / _grad_o_f32 of another build of the library, bound like _lib does."""
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    for name in ("rtk_bce_stream_rows_f32", "rtk_bce_stream_grad_o_f32", "rtk_bce_stream_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = rt._lib.SIGNATURES[name]
    return lib


def run_abi(params, flt, ids, iters, rounds, warm, yard_path):
    lib = rt._lib.load()
    yard = whole_entry_points(yard_path) if yard_path else lib
    core, R, S, O = params
    n_loc = N_ENT // P_RANKS
    col0 = BLOCK * n_loc
    O_blk = O[col0:col0 + n_loc].contiguous()
    c = O.shape[1]
    f = flt.features[ids]
    with torch.no_grad():
        v, qp = rt.query_vectors(core, R, S, f[:, 0].contiguous(), f[:, 1].contiguous(), packed=True)
    slot = flt.slot_of_item[ids].contiguous()
    obj_shift = (flt.pair_obj - col0).contiguous()
    max_pos = B * flt.max_list
    flags = rt._lib.RTK_SCORE_SIGMOID | rt._lib.RTK_SCORE_SIGMOID_FAST
    ws = torch.zeros(lib.rtk_bce_stream_part_workspace_bytes(B, n_loc, c, max_pos), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= yard.rtk_bce_stream_workspace_bytes(B, n_loc, c, max_pos)
    sc = torch.tensor([1.0 / (B * N_ENT)], device="cuda")
    sp = torch.cuda.current_stream().cuda_stream

    def buffers():
        return (torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty((B, c), device="cuda"),
                torch.empty((n_loc, c), device="cuda"))
    out_y, out_b = buffers(), buffers()
    csr = (slot.data_ptr(), flt.pair_ptr.data_ptr())

    def rows_yard(eps=EPS):
        rt._lib.check(yard.rtk_bce_stream_rows_f32(qp.data_ptr(), B, c, O_blk.data_ptr(), n_loc, *csr, obj_shift.data_ptr(),
                                                   eps, flags, out_y[0].data_ptr(), out_y[1].data_ptr(), ws.data_ptr(),
                                                   ws.numel(), sp), "rows (yardstick)")

    def go_yard(eps=EPS):
        rt._lib.check(yard.rtk_bce_stream_grad_o_f32(qp.data_ptr(), v.data_ptr(), B, c, O_blk.data_ptr(), n_loc, *csr,
                                                     obj_shift.data_ptr(), max_pos, eps, flags, sc.data_ptr(),
                                                     out_y[2].data_ptr(), ws.data_ptr(), ws.numel(), sp), "grad_o (yardstick)")

    def rows_blk(eps=EPS):
        rt._lib.check(lib.rtk_bce_stream_rows_part_f32(qp.data_ptr(), B, c, O_blk.data_ptr(), n_loc, col0, N_ENT, *csr,
                                                       flt.pair_obj.data_ptr(), eps, flags, out_b[0].data_ptr(),
                                                       out_b[1].data_ptr(), ws.data_ptr(), ws.numel(), sp), "rows_part")

    def go_blk(eps=EPS):
        rt._lib.check(lib.rtk_bce_stream_grad_o_part_f32(qp.data_ptr(), v.data_ptr(), B, c, O_blk.data_ptr(), n_loc, col0,
                                                         N_ENT, *csr, flt.pair_obj.data_ptr(), max_pos, eps, flags,
                                                         sc.data_ptr(), out_b[2].data_ptr(), ws.data_ptr(), ws.numel(), sp),
                      "grad_o_part")

    # eps = 0: no smoothing term, so the block of a 1 M matrix and the 125 000-entity matrix are the same problem
    for fn in (rows_yard, go_yard, rows_blk, go_blk):
        fn(0.0)
    torch.cuda.synchronize()
    same = [torch.equal(a, b) for a, b in zip(out_y, out_b)]
    n_own = int(((flt.pair_obj >= col0) & (flt.pair_obj < col0 + n_loc)).sum())
    print(f"== abi: rows [{col0}, {col0 + n_loc}) of {N_ENT}, B {B}, c {c}, max_pos {max_pos}; {n_own} of "
          f"{flt.pair_obj.numel()} CSR entries in the block; yardstick library: {yard_path or 'this build'}")
    print(f"  eps = 0: rows / dv / gO bit-equal to the whole-matrix call on the same rows: {same}")
    res = {}
    for _ in range(rounds):                                   # alternated: yardstick, block, yardstick, block, ...
        for name, fn in (("rows  yardstick (n_ent 125 000)", rows_yard), ("rows  block form", rows_blk),
                         ("gradO yardstick (n_ent 125 000)", go_yard), ("gradO block form", go_blk)):
            res.setdefault(name, []).append(timed(fn, warm, iters))
    for name, ts in res.items():
        print(f"  {name:34}: " + "  ".join(f"{t:8.3f}" for t in ts) + f"  ms (median of {iters} per round); "
              f"spread {max(ts) - min(ts):.3f}")
    assert int(ws[:4].view(torch.int32).item()) == 0


def run_step(params, flt, ids, iters, rounds, warm, loss_name="bce"):
    core, R, S, O = [p.requires_grad_(True) for p in params]
    n_loc = N_ENT // P_RANKS
    col0 = BLOCK * n_loc
    O_blk = O.detach()[col0:col0 + n_loc].clone().requires_grad_(True)
    f = flt.features[ids]
    h, r = f[:, 0].contiguous(), f[:, 1].contiguous()
    ce = loss_name == "ce"
    lse = None
    if ce:                                                        # the global lse, once and untimed
        Od = O.detach()
        parts = [rt.ce_partials_block_1vN(core, R, S, Od[k * n_loc:(k + 1) * n_loc], k * n_loc, N_ENT, h, r, flt, ids,
                                          label_smoothing=EPS) for k in range(P_RANKS)]
        lse = rt.ce_merge_lse([p[0] for p in parts], [p[1] for p in parts])

    def step_whole():
        for p in (core, R, S, O):
            p.grad = None
        whole = rt.ce_loss_1vN if ce else rt.bce_loss_1vN
        loss = whole(core, R, S, O, h, r, flt, ids, label_smoothing=EPS, matrix_free=True)
        loss.backward()
        return loss

    def step_block():
        for p in (core, R, S, O_blk):
            p.grad = None
        if ce:
            loss = rt.ce_loss_block_1vN(core, R, S, O_blk, col0, N_ENT, h, r, flt, ids, label_smoothing=EPS, lse=lse)
        else:
            loss = rt.bce_loss_block_1vN(core, R, S, O_blk, col0, N_ENT, h, r, flt, ids, label_smoothing=EPS)
        loss.backward()
        return loss

    block_name = f"one block of 8, {loss_name}_loss_block_1vN"
    print(f"== step ({loss_name}): forward + backward, B {B}, rank {RANK}; whole matrix N {N_ENT} against one block of "
          f"{n_loc} rows")
    res = {}
    for _ in range(rounds):
        for name, fn in (("whole matrix, matrix_free=True", step_whole), (block_name, step_block)):
            res.setdefault(name, []).append(timed(fn, warm, iters))
    peaks = {"whole matrix, matrix_free=True": peak_of(step_whole), block_name: peak_of(step_block)}
    for name, ts in res.items():
        print(f"  {name:36}: " + "  ".join(f"{t:8.3f}" for t in ts) + f"  ms; peak over the live bytes {peaks[name]:8.1f} MB")
    a, b = (float(np.median(res[k])) for k in res)
    print(f"  ratio block / whole: {b / a:.3f} (1/8 of the sweeps plus the full stage 1 and positives)")
    print(f"  loss {step_whole().item():.6f}; the block's share {step_block().item():.6f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="both", choices=("abi", "step", "both"))
    ap.add_argument("--loss", default="bce", choices=("bce", "ce"))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    flt = rt.DeviceFilter(SyntheticPairs(N_ENT, N_REL, B, 1), "cuda")
    ids = torch.arange(B).cuda()
    params = [torch.from_numpy(x).cuda() for x in gen.make_params(N_ENT, N_REL, RANK, 322)]
    if a.loss == "ce" and a.part == "abi":
        ap.error("--loss ce measures the step part only")
    if a.part in ("abi", "both") and a.loss == "bce":
        run_abi(params, flt, ids, a.iters, a.rounds, a.warmup, a.yardstick_lib)
    if a.part in ("step", "both"):
        run_step(params, flt, ids, a.iters, a.rounds, a.warmup, a.loss)
