"""Cases of the stage-1 backward without the (B, a*b) intermediates (``rtk_query_vectors_bwd_stream_*``,
csrc/rtk_query_bwd_stream.hip), and a float64 model of its kernels with switchable faults.

The cases are ``exact_cases.BwdCase`` objects: operands from ``exact_cases.bwd_operands``, references from ``bwd_ref``,
bounds from ``bwd_bounds(..., splits=1)`` (g_core is one chain over the batch here: no split-K).  The shapes walk the
edges of the kernel's tiles: 128 queries x 128 columns of b per workgroup, 32 queries per wave, k-tiles of 16, the
vector / scalar row loads (c % 4), one to several tiles in every direction.

``model`` walks the same tiles in float64.  On the exact cases any summation order gives the float64 reference, so the
model equals ``bwd_ref`` there, and each fault (``MUTANTS``) must change the result of at least one exact case --
tests/test_stage1_bwd_stream_cases_host.py proves both without a GPU.
"""
import numpy as np

import exact_cases as ec

TILE_Q, TILE_B, TILE_K = 128, 128, 16      # the kernel's tile: queries, columns of b, k


def _cases():
    b, cs = ec._b, []
    for w in (1, 31, 33, 127, 128, 129, 257):
        cs.append(b(f"st_b{w}", 140, 3, w, 8, 6, 30, regime="small", branch="b edges"))
    for B in (1, 31, 33, 127, 128, 129, 257):
        cs.append(b(f"st_B{B}", B, 5, 40, 8, 4, 50, regime="wide12", wide="dv", branch="B edges"))
    for c in (1, 2, 7, 15, 16, 17, 33, 140):
        cs.append(b(f"st_c{c}", 130, 4, 36, c, 5, 40, regime="small", branch="K edges (c % 4 != 0: scalar row loads)"))
    for a in (1, 2, 31, 33, 129):
        cs.append(b(f"st_a{a}", 70, a, 20, 8, 5, 40, regime="wide12", wide="core", branch="a edges"))
    cs.append(b("st_tiles", 300, 40, 300, 24, 9, 500, regime="wide12", wide="core", branch="several tiles in every direction"))
    cs.append(b("st_wide12_core", 200, 5, 257, 12, 4, 50, regime="wide12", wide="core", branch="12-bit core"))
    cs.append(b("st_wide20_dv_tiny", 12, 2, 3, 2, 20, 20, regime="wide20", wide="dv", rel_ids=("distinct",),
                sub_ids=("distinct",), branch="20-bit dv"))
    cs.append(b("st_wide20_core_tiny", 12, 3, 2, 2, 20, 20, regime="wide20", wide="core", rel_ids=("distinct",),
                sub_ids=("distinct",), branch="20-bit core"))
    cs.append(b("st_ids_one", 700, 2, 130, 4, 3, 10, regime="small", sub_ids=("one", 9), rel_ids=("one", 0),
                branch="one id on every query"))
    cs.append(b("st_ids_distinct", 257, 9, 33, 8, 300, 4000, regime="wide12", wide="core", rel_ids=("distinct",),
                sub_ids=("distinct",), branch="all ids distinct"))
    cs.append(b("st_real_wn18rr", 512, 10, 200, 200, 11, 3000, regime="real", branch="real values, WN18RR rank"))
    cs.append(b("st_real_c5_widths", 33, 8, 512, 512, 6, 100, regime="real", branch="real values, C5 widths: four b-tiles"))
    cs.append(b("st_real_pow2", 256, 33, 130, 16, 6, 500, regime="real_pow2", sub_ids=("lists", (3, (200,), 1)),
                branch="real values, per-row powers of two, one list of 200"))
    return cs


CASES = _cases()
MUTANTS = ("last_k_tile", "last_i", "b_tile_partial", "neighbour_row", "rows_past_B")


def workspace_model(B, a, b):
    """Bytes of the workspace as the header states them (256-byte aligned pieces)."""
    up = lambda x: -(-x // 256) * 256        # noqa: E731
    n_bt = -(-b // TILE_B)
    return 2 * up(4 * B * a) + 2 * up(4 * B * b) + up(4 * n_bt * B * a)


def model(core, R, S, dv, rel, sub, mutant=None):
    """(g_core, g_R, g_S) in float64, tile by tile as stream_rows_kernel forms them.  ``mutant``: one of MUTANTS.
      last_k_tile     the last k-tile of every W tile is dropped
      last_i          the i loop stops one short
      b_tile_partial  the finish step leaves out the last b-tile's partial of rows_R
      neighbour_row   W meets the S / R row of the next query of the tile
      rows_past_B     the tiles' padding is read as GARBAGE instead of zeros: rows of dv past B (those queries then count,
                      with the last query's ids) and columns of the core and of S past b"""
    assert mutant is None or mutant in MUTANTS
    a, b, c = core.shape
    B = dv.shape[0]
    core, R, S, dv = [np.asarray(x, dtype=np.float64) for x in (core, R, S, dv)]
    rel, sub = np.asarray(rel), np.asarray(sub)
    pad = ec.GARBAGE if mutant == "rows_past_B" else 0.0
    Bp, bp = -(-B // TILE_Q) * TILE_Q, -(-b // TILE_B) * TILE_B
    n_rows = Bp if mutant == "rows_past_B" else B                  # the queries that reach the outputs
    relp = np.concatenate([rel, np.full(Bp - B, rel[-1])])
    subp = np.concatenate([sub, np.full(Bp - B, sub[-1])])
    dvp = np.full((Bp, c), pad)
    dvp[:B] = dv
    Rg = R[relp]
    Sg = np.full((Bp, bp), pad)
    Sg[:, :b] = S[subp]
    G = np.full((a, bp, c), pad)
    G[:, :b] = core
    shift = 1 if mutant == "neighbour_row" else 0
    k_tiles = list(range(0, c, TILE_K))
    if mutant == "last_k_tile":
        k_tiles = k_tiles[:-1]
    n_i = a - 1 if mutant == "last_i" else a
    n_bt = bp // TILE_B
    rows_S = np.zeros((Bp, bp))
    part = np.zeros((n_bt, Bp, a))
    for q0 in range(0, Bp, TILE_Q):
        q = slice(q0, q0 + TILE_Q)
        Rt, St = np.roll(Rg[q], -shift, axis=0), np.roll(Sg[q], -shift, axis=0)
        for bt in range(n_bt):
            j = slice(bt * TILE_B, (bt + 1) * TILE_B)
            for i in range(n_i):
                W = np.zeros((TILE_Q, TILE_B))
                for k0 in k_tiles:
                    W += dvp[q, k0:k0 + TILE_K] @ G[i, j, k0:k0 + TILE_K].T
                rows_S[q, j] += W * Rt[:, i:i + 1]
                part[bt, q, i] = np.sum(W * St[:, j], axis=1)
    rows_R = np.zeros((Bp, a))
    for bt in range(n_bt - 1 if mutant == "b_tile_partial" else n_bt):
        rows_R += part[bt]
    X = (Rg[:n_rows, :, None] * Sg[:n_rows, None, :b]).reshape(n_rows, a * b)
    g_core = (X.T @ dvp[:n_rows]).reshape(a, b, c)
    g_R, g_S = np.zeros(R.shape), np.zeros(S.shape)
    np.add.at(g_R, relp[:n_rows], rows_R[:n_rows])
    np.add.at(g_S, subp[:n_rows], rows_S[:n_rows, :b])
    return g_core, g_R, g_S
