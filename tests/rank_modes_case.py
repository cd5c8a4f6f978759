"""The operands on which the three modes of the matrix-free count (stable, stable + BCE, tie counts) are compared: the
smallest shapes that reach every branch of step 2 (test support for tests/test_gpu_rank_modes.py and
tools/rank_digest.py; needs the GPU).

  shapes   f32 N = 1500, c = 20, B = 70; bf16 N = 777, c = 18 (rows too short for vector loads), B = 70: a batch that is
           no multiple of 32 and takes three finish workgroups; 12 entity tiles at f32
  blocks   the whole range, and at f32 [0, 100) + [100, 1300) + [1300, 1500): a block below one 128-row tile (the query
           tiles are cut into ranges) and one of 10 tiles (the finish pass's 8-apart slot loop takes a second trip)
  filter   query 0: 300 entries (two trips of the 8 filter waves) with its own target and entries in every block;
           query 1: an empty list; query 2: slot -1; the others up to 40 entries
  ties     query 3: its target's row of O copied to the ids one below and one above (bit-equal probabilities);
           query 4: a subject row scaled until the row minimum of the probabilities is exactly 0, the target on it
"""
import numpy as np
import torch

from test_gpu_rank import Flt, _flags, _problem, _stored_scores

SHAPES = {"f32": (1500, 20, 70), "bf16": (777, 18, 70)}
PARTITION_F32 = ((0, 100), (100, 1300), (1300, 1500))
LONG_LIST = 300


class Case:
    pass


def build(rt, kind, mode):
    """The case of ``kind`` ("f32" / "bf16") under the logistic ``mode``: operands, packed queries, targets, the filter
    stand-in with its per-query lists, the stored kernel's probabilities (numpy) and the blocks to count on."""
    N, c, B = SHAPES[kind]
    dtype = torch.float32 if kind == "f32" else torch.bfloat16
    core, R, S, O, h, r, t = _problem(N, c, B, 1000 + c, 1.0 if kind == "f32" else 8.0, dtype=dtype)
    rng = np.random.default_rng(N)
    S, O, h, t = S.clone(), O.clone(), h.clone(), t.clone()
    # query 4: a subject of its own, scaled so that its probabilities saturate
    free = sorted(set(range(N)) - set(h.cpu().tolist()))
    h[4] = free[0]
    S[h[4]] *= 1e4
    # query 3: two bit-equal competitors, one id below and one above the target
    t[3] = min(max(int(t[3]), 1), N - 2)
    O[t[3] - 1] = O[t[3]]
    O[t[3] + 1] = O[t[3]]
    _, qp = rt.query_vectors(core, R, S, h, r, packed=True)
    P = _stored_scores(rt, qp, B, O, _flags(rt, mode))
    t[4] = P[4].argmin()
    tn = t.cpu().numpy()
    edges = [5, 50, N - 100, N - 50]                                 # in the first and in the last block
    lists, slots = [], []
    for d in range(B):
        if d == 2:
            slots.append(-1)
            continue
        if d == 0:
            rest = [j for j in rng.permutation(N).tolist() if j != tn[0] and j not in edges]
            objs = [int(tn[0])] + edges + rest[:LONG_LIST - 1 - len(edges)]
        elif d == 1:
            objs = []
        else:                                                        # (query 4: enough entries for some to be non-zero)
            m = 20 if d == 4 else int(rng.integers(1, 40))
            objs = [j for j in rng.choice(N, size=m, replace=False).tolist() if j != tn[d]]
            if d % 3 == 0:
                objs.append(int(tn[d]))
        slots.append(len(lists))
        lists.append(sorted(objs))
    cs = Case()
    cs.kind, cs.mode, cs.N, cs.c, cs.B = kind, mode, N, c, B
    cs.O, cs.qp, cs.t, cs.P, cs.Pn, cs.tn = O, qp, t, P, P.cpu().numpy(), tn
    cs.flt = Flt(lists, slots)
    cs.lists = [lists[s] if s >= 0 else None for s in slots]
    cs.blockings = [((0, N),)] + ([PARTITION_F32] if kind == "f32" else [])
    return cs
