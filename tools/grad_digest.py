#!/usr/bin/env python3
"""SHA-256 of every output and every gradient of the differentiable ops of r-tucker_amd/ops.py, on fixed seeds: score_1vN
and score_candidates with and without the logistic, score_triples, bce_loss_1vN (stored matrix with FUSED_BCE on and off,
and matrix_free), ce_loss_1vN (both forms), the two block losses on rows [32, 96), relation_logits and relation_ce_loss.
Shapes are the smallest that reach every branch of the host code: N = 130 (not a multiple of the 32-float row pitch),
c = 20, a = 3 at B = 70 and B = 1; N = 1100 (_splits_for gives split-K); c = 520 at B = 5 (the unpacked rtk_score_f32
stage 2 and with it the unfused BCE); B = 0; fp32 and bf16 operands; distinct S and O and S is O; one operand requiring a
gradient at a time and all of them; BACKWARD_GEMM "split_fp16" and "f32".  A call that raises prints ``raises <type>``.
One line per tensor; two trees of the Python host compute the same thing on one library when the lines are equal:

    R_TUCKER_AMD_LIB=/path/to/librtucker_hip.so python tools/grad_digest.py --tree /path/to/other/checkout > a.txt
    R_TUCKER_AMD_LIB=/path/to/librtucker_hip.so python tools/grad_digest.py > b.txt && diff a.txt b.txt

    --summary     one line per shape, dtype and flavour instead: its number of lines, how many of them read "raises",
                  and the SHA-256 of the lines (9112 lines become 20; what profiles/ keeps)
"""
import hashlib
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:]:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
import r_tucker_amd as rt  # noqa: E402
from r_tucker_amd import ops  # noqa: E402

N_REL, EPS = 5, 0.1
# (tag, N, rank, B)
SHAPES = (("N130 B70", 130, (3, 20, 20), 70), ("N130 B1", 130, (3, 20, 20), 1), ("N1100 B70", 1100, (3, 20, 20), 70),
          ("c520 B5", 130, (3, 520, 520), 5), ("N130 B0", 130, (3, 20, 20), 0))
NAMES = ("core", "R", "S", "O")
SUMMARY = "--summary" in sys.argv[1:]
LINES = []


def emit(line):
    LINES.append(line)
    if not SUMMARY:
        print(line, flush=True)


def summarise(group, lines):
    text = "".join(line + "\n" for line in lines)
    return (f"{group}: {len(lines)} lines, {sum(': raises ' in line for line in lines)} raises, "
            f"sha256 {hashlib.sha256(text.encode()).hexdigest()}")


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def problem(N, rank, B, dtype, shared, seed):
    """Operand values, queries, a CSR of known objects (lists of 0 to 4 entries, the second one empty), candidates."""
    g = torch.Generator().manual_seed(seed)
    shapes = (rank, (N_REL, rank[0]), (N, rank[1]), (N, rank[2]))
    values = [(0.4 * torch.randn(s, generator=g)).to(dtype).cuda() for s in shapes]
    if shared:
        values[3] = values[2]
    rnd = lambda hi, *shape: torch.randint(0, hi, shape, generator=g).cuda()  # noqa: E731
    h, r, t, rel = rnd(N, B), rnd(N_REL, B), rnd(N, B), rnd(N_REL, B)
    lens = torch.randint(0, 5, (B,), generator=g)
    lens[:1], lens[1:2] = 2, 0
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).cuda()
    flt = SimpleNamespace(slot_of_item=torch.arange(B).cuda(), pair_ptr=ptr, pair_obj=rnd(N, int(lens.sum())), max_list=4)
    return SimpleNamespace(values=values, h=h, r=r, t=t, rel=rel, flt=flt, ids=torch.arange(B).cuda(), cand=rnd(N, B, 7),
                           B=B, N=N, shared=shared)


def block_ce(p, c, R, S, O):
    """ce_loss_block_1vN on rows [32, 96) with the global lse of the three blocks' partials."""
    with torch.no_grad():
        parts = [rt.ce_partials_block_1vN(c, R, S, O[lo:hi], lo, p.N, p.h, p.r, p.flt, p.ids, EPS)
                 for lo, hi in ((0, 32), (32, 96), (96, p.N))]
        lse = rt.ce_merge_lse([m for m, _, _ in parts], [s for _, s, _ in parts])
    return rt.ce_loss_block_1vN(c, R, S, O[32:96], 32, p.N, p.h, p.r, p.flt, p.ids, EPS, lse=lse)


def fused(on, fn):
    def call(p, *operands):
        ops.FUSED_BCE = on
        try:
            return fn(p, *operands)
        finally:
            ops.FUSED_BCE = True
    return call


def bce(p, c, R, S, O, **kw):
    return rt.bce_loss_1vN(c, R, S, O, p.h, p.r, p.flt, p.ids, EPS, **kw)


OPS = (
    ("score_1vN sigmoid", lambda p, *o: rt.score_1vN(*o, p.h, p.r, sigmoid=True)),
    ("score_1vN logits", lambda p, *o: rt.score_1vN(*o, p.h, p.r, sigmoid=False)),
    ("bce_loss_1vN fused=1", fused(True, bce)),
    ("bce_loss_1vN fused=0", fused(False, bce)),
    ("bce_loss_1vN matrix_free", lambda p, *o: bce(p, *o, matrix_free=True)),
    ("ce_loss_1vN matrix", lambda p, *o: rt.ce_loss_1vN(*o, p.h, p.r, p.flt, p.ids, EPS)),
    ("ce_loss_1vN matrix_free", lambda p, *o: rt.ce_loss_1vN(*o, p.h, p.r, p.flt, p.ids, EPS, matrix_free=True)),
    ("bce_loss_block_1vN [32, 96)", lambda p, c, R, S, O: rt.bce_loss_block_1vN(c, R, S, O[32:96], 32, p.N, p.h, p.r, p.flt,
                                                                                p.ids, EPS)),
    ("ce_loss_block_1vN [32, 96) lse", block_ce),
    ("score_candidates sigmoid", lambda p, *o: rt.score_candidates(*o, p.h, p.r, p.cand, sigmoid=True)),
    ("score_candidates logits", lambda p, *o: rt.score_candidates(*o, p.h, p.r, p.cand, sigmoid=False)),
    ("score_triples", lambda p, *o: rt.score_triples(*o, p.h, p.r, p.t)),
    ("relation_logits", lambda p, *o: rt.relation_logits(*o, p.h, p.t)),
    ("relation_ce_loss", lambda p, *o: rt.relation_ce_loss(*o, p.h, p.t, p.rel, label_smoothing=EPS)),
)


def run(tag, p, name, fn, wanted):
    n_leaves = 3 if p.shared else 4
    leaves = [v.clone().requires_grad_(i in wanted) for i, v in enumerate(p.values[:n_leaves])]
    try:
        out = fn(p, *(leaves + [leaves[2]] if p.shared else leaves))
        if out.dim() == 0:
            (out * 1.75).backward()
        else:
            out.backward(torch.randn(out.shape, generator=torch.Generator().manual_seed(11)).cuda())
        torch.cuda.synchronize()
        rt.check_device_errors()
    except Exception as e:  # noqa: BLE001  (a refusal is part of the record)
        emit(f"{tag} | {name}: raises {type(e).__name__}")
        print(f"# {tag} | {name}: {str(e).splitlines()[0] if str(e) else ''}", file=sys.stderr)
        return
    emit(f"{tag} | {name}: out {tuple(out.shape)} {sha(out)}")
    for i, leaf in enumerate(leaves):
        label = "E" if p.shared and i == 2 else NAMES[i]
        emit(f"{tag} | {name}: g_{label} {'None' if leaf.grad is None else sha(leaf.grad)}")


if __name__ == "__main__":
    assert torch.cuda.is_available()
    rt._lib.load()
    print(f"# library {rt._lib.LIB_PATH}, rtk_version {rt._lib.load().rtk_version()}", file=sys.stderr)
    for (stag, N, rank, B) in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for shared in (False, True):
                p = problem(N, rank, B, dtype, shared, seed=N + 7 * B + rank[2])
                n_leaves = 3 if shared else 4
                for wanted in [tuple(range(n_leaves))] + [(i,) for i in range(n_leaves)]:
                    for gemm in ("split_fp16", "f32"):
                        ops.BACKWARD_GEMM = gemm
                        tag = (f"{stag} {'bf16' if dtype == torch.bfloat16 else 'f32'} {'S_is_O' if shared else 'asym'} "
                               f"grad={'+'.join(NAMES[i] for i in wanted)} gemm={gemm}")
                        for name, fn in OPS:
                            run(tag, p, name, fn, wanted)
                if SUMMARY:
                    print(summarise(tag.split(" grad=")[0], LINES), flush=True)
                LINES.clear()
    ops.BACKWARD_GEMM = "split_fp16"
