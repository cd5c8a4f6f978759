#!/usr/bin/env python3
"""SHA-256 of every output of the ranking entries (csrc/rtk_score_rank.hip, csrc/rtk_rank.hip), on fixed seeds, through
the C entries, on the operands of tests/rank_modes_case.py (f32 N = 1500, c = 20, B = 70 in both logistic modes, bf16
N = 777, c = 18; the whole range and the f32 partition [0, 100) + [100, 1300) + [1300, 1500); a CSR list of 300 entries,
an empty one, a slot of -1; planted ties): pt, counts and bce_rows of rtk_score_rank_counts_* without and with BCE, ranks
and bce_rows of rtk_score_rank_*, greater / equal of rtk_score_rank_tie_counts_*, the stored-matrix entries on the stored
kernel's scores of the same operands, acc5 / acc13 of the two metrics entries after two accumulating calls.  One line
per output; two builds of the library compute the same thing when the lines are equal:

    R_TUCKER_AMD_LIB=/path/to/other/librtucker_hip.so python tools/rank_digest.py > a.txt
    python tools/rank_digest.py > b.txt && diff a.txt b.txt

    python tools/rank_digest.py --sizes     the workspace-size functions on a grid of arguments instead (needs no GPU)
"""
import hashlib
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import r_tucker_amd as rt  # noqa: E402


def stream():
    return torch.cuda.current_stream().cuda_stream


def report(name, t):
    torch.cuda.synchronize()
    print(f"{name:58s} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}", flush=True)


def ok(lib, rc):
    assert rc == 0, lib.rtk_last_error_string()


def new(B, dtype):
    """An output the entry has to write in full: NaN / -1 where it does not."""
    return torch.full((B,), float("nan") if dtype.is_floating_point else -1, dtype=dtype, device="cuda")


def matrix_free(lib, cs, tag):
    B, N, c, sfx = cs.B, cs.N, cs.c, "_" + cs.kind
    dcode = 0 if cs.kind == "f32" else 1
    flags = rt.ops._score_flags(True, cs.mode, torch.float32, cs.kind == "bf16")
    csr = (cs.flt.slot_of_item.data_ptr(), cs.flt.pair_ptr.data_ptr(), cs.flt.pair_obj.data_ptr())
    fn = {n: getattr(lib, f"rtk_score_rank{n}{sfx}") for n in ("", "_targets", "_counts", "_tie_counts")}
    nws = lib.rtk_score_rank_workspace_bytes(dcode, B, N, c)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    for want_bce in (False, True):
        ranks, bce = new(B, torch.int32), new(B, torch.float64)
        ok(lib, fn[""](cs.qp.data_ptr(), B, c, cs.O.data_ptr(), N, cs.t.data_ptr(), *csr, flags, ranks.data_ptr(),
                       bce.data_ptr() if want_bce else None, ws.data_ptr(), nws, stream()))
        report(f"{tag} score_rank bce={int(want_bce)} ranks", ranks)
        if want_bce:
            report(f"{tag} score_rank bce=1 bce_rows", bce)
    for blocks in cs.blockings:
        pts = []
        for lo, hi in blocks:
            nws = lib.rtk_score_rank_part_workspace_bytes(dcode, B, hi - lo, c)
            ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
            pts.append(new(B, torch.float32))
            ok(lib, fn["_targets"](cs.qp.data_ptr(), B, c, cs.O[lo:hi].data_ptr(), hi - lo, lo, N, cs.t.data_ptr(), flags,
                                   pts[-1].data_ptr(), ws.data_ptr(), nws, stream()))
        pt = torch.stack(pts).max(dim=0).values.contiguous()
        report(f"{tag} blocks={len(blocks)} pt", pt)
        for lo, hi in blocks:
            a = (cs.qp.data_ptr(), B, c, cs.O[lo:hi].data_ptr(), hi - lo, lo, N, pt.data_ptr(), cs.t.data_ptr(), *csr, flags)
            nws = lib.rtk_score_rank_part_workspace_bytes(dcode, B, hi - lo, c)
            ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
            for want_bce in (False, True):
                counts, bce = new(B, torch.int32), new(B, torch.float64)
                ok(lib, fn["_counts"](*a, counts.data_ptr(), bce.data_ptr() if want_bce else None, ws.data_ptr(), nws, stream()))
                report(f"{tag} [{lo}, {hi}) counts bce={int(want_bce)} counts", counts)
                if want_bce:
                    report(f"{tag} [{lo}, {hi}) counts bce=1 bce_rows", bce)
            nws = lib.rtk_score_rank_ties_workspace_bytes(dcode, B, hi - lo, c)
            ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
            greater, equal = new(B, torch.int32), new(B, torch.int32)
            ok(lib, fn["_tie_counts"](*a, greater.data_ptr(), equal.data_ptr(), ws.data_ptr(), nws, stream()))
            report(f"{tag} [{lo}, {hi}) tie_counts greater", greater)
            report(f"{tag} [{lo}, {hi}) tie_counts equal", equal)


def stored(lib, cs, tag):
    """The stored-matrix entries on the stored kernel's scores, and the metrics entries on their outputs."""
    B, N, P = cs.B, cs.N, cs.P
    csr = (cs.flt.slot_of_item.data_ptr(), cs.flt.pair_ptr.data_ptr(), cs.flt.pair_obj.data_ptr())
    ranks, bce = new(B, torch.int32), new(B, torch.float64)
    ok(lib, lib.rtk_filtered_rank_f32(P.data_ptr(), B, N, P.stride(0), cs.t.data_ptr(), *csr, ranks.data_ptr(), bce.data_ptr(),
                                      stream()))
    report(f"{tag} filtered_rank ranks", ranks)
    report(f"{tag} filtered_rank bce_rows", bce)
    greater = equal = None
    for blocks in cs.blockings:
        pts = []
        for lo, hi in blocks:
            pts.append(new(B, torch.float32))
            ok(lib, lib.rtk_target_scores_f32(P[:, lo:].data_ptr(), B, hi - lo, P.stride(0), lo, cs.t.data_ptr(),
                                              pts[-1].data_ptr(), stream()))
            report(f"{tag} [{lo}, {hi}) target_scores pt", pts[-1])
        pt = torch.stack(pts).max(dim=0).values.contiguous()
        for lo, hi in blocks:
            a = (P[:, lo:].data_ptr(), B, hi - lo, P.stride(0), lo, pt.data_ptr(), cs.t.data_ptr(), *csr)
            counts, pbce = new(B, torch.int32), new(B, torch.float64)
            ok(lib, lib.rtk_filtered_rank_partial_f32(*a, counts.data_ptr(), pbce.data_ptr(), stream()))
            report(f"{tag} [{lo}, {hi}) filtered_rank_partial counts", counts)
            report(f"{tag} [{lo}, {hi}) filtered_rank_partial bce_rows", pbce)
            g, e = new(B, torch.int32), new(B, torch.int32)
            ok(lib, lib.rtk_filtered_tie_counts_partial_f32(*a, g.data_ptr(), e.data_ptr(), stream()))
            report(f"{tag} [{lo}, {hi}) filtered_tie_counts_partial greater", g)
            report(f"{tag} [{lo}, {hi}) filtered_tie_counts_partial equal", e)
            if greater is None:
                greater, equal = g, e                               # the whole range's
    acc5 = torch.zeros(5, dtype=torch.float64, device="cuda")
    acc13 = torch.zeros(13, dtype=torch.float64, device="cuda")
    for _ in range(2):
        ok(lib, lib.rtk_rank_metrics_scaled_f64(ranks.data_ptr(), bce.data_ptr(), B, 1.0 / (B * N), acc5.data_ptr(), stream()))
        ok(lib, lib.rtk_tie_metrics_f64(greater.data_ptr(), equal.data_ptr(), B, acc13.data_ptr(), stream()))
    ok(lib, lib.rtk_rank_metrics_f64(ranks.data_ptr(), None, B, acc5.data_ptr(), stream()))
    report(f"{tag} rank_metrics acc5", acc5)
    report(f"{tag} tie_metrics acc13", acc13)


def sizes(lib):
    """The workspace-size functions of csrc/rtk_score_rank.hip on a grid of arguments, refused shapes included."""
    batches = (-1, 0, 1, 31, 32, 33, 70, 512, 8192, 100000, (1 << 31) - 33, (1 << 31) - 32, 1 << 31)
    ns = (-5, 0, 1, 100, 127, 128, 129, 777, 1500, 40943, 1000000, (1 << 31) - 65, (1 << 31) - 64, 1 << 32)
    cs = (-4, 0, 1, 4, 18, 20, 200, 208, 210, 212, 512, 513)
    for name in ("rtk_score_rank_workspace_bytes", "rtk_score_rank_part_workspace_bytes", "rtk_score_rank_ties_workspace_bytes"):
        f = getattr(lib, name)
        h, n = hashlib.sha256(), 0
        for a in itertools.product((0, 1, 2), batches, ns, cs):
            h.update(f"{a} {f(*a)}\n".encode())
            n += 1
        print(f"{name:58s} {n} tuples {h.hexdigest()}  e.g. (0, 512, 40943, 200) -> {f(0, 512, 40943, 200)}")


if __name__ == "__main__":
    lib = rt._lib.load()
    print(f"# {os.path.relpath(rt._lib.LIB_PATH, ROOT)}", file=sys.stderr)
    if "--sizes" in sys.argv[1:]:
        sizes(lib)
        sys.exit(0)
    assert torch.cuda.is_available()
    import rank_modes_case  # noqa: E402
    for kind, mode in (("f32", "fast"), ("f32", "exact"), ("bf16", "exact")):
        cs = rank_modes_case.build(rt, kind, mode)
        report(f"{kind} {mode} stored scores", cs.P)
        matrix_free(lib, cs, f"{kind} {mode}")
        stored(lib, cs, f"{kind} {mode}")
