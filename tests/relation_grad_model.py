"""A plain numpy model of the gradients of relation prediction (test support, no GPU, no library).  With the notation
of tests/relation_model.py and a given dZ (B, n_rel):

    du = dZ . R                                             (B, a)
    gR = dZ^T . u                                           (n_rel, a)
    rS[d, j] = sum_i du[d, i] * sum_k G[i, j, k] O[t_d, k]      gS[e, :] = sum_{d: h_d = e} rS[d, :]
    rO[d, k] = sum_i du[d, i] * sum_j G[i, j, k] S[h_d, j]      gO[e, :] = sum_{d: t_d = e} rO[d, :]
    gG[i, j, k] = sum_d du[d, i] S[h_d, j] O[t_d, k]

in float64 on the operands as stored, and the error bounds of the device path.  Every term of a bound is either a
bound tests/relation_model.py already states, or the fp32 accumulation bound  acc(n, T) = (n + 2) 2^-24 T  of a sum of n
rounded products (or n terms) whose magnitudes add up to T, in any order; nothing is fitted.

Derivation.

  rows   rtk_pair_rows_f32 computes rows[d, j] = sum_i w[d, i] * sum_k core[i, j, k] X[x_d, k].  That is the forward's
         sweep on the core with its first two axes exchanged (core'[j, i, k] = core[i, j, k]), w in the place of S[h]
         (query d reads row d) and X[x_idx] in the place of O[t]: the same instructions, so the forward's own bound,
         relation_model.u_bounds(core', w, X, arange(B), x_idx, False), holds.  It depends on w through |w| alone and
         grows with it.
  du     one fp32 chain of n_rel products: tau_du = acc(n_rel, |dZ| . |R|).
  gR     the device multiplies dZ by ITS u, which tau_u (relation_model) places within tau_u of u64:
         tau_gR = |dZ|^T . tau_u + acc(B, |dZ|^T . |u64|).
  rS/rO  the device's sweep is given ITS du, du' with |du' - du64| <= tau_du, so |du'| <= |du64| + tau_du.  Its result is
         within the rows bound AT |du64| + tau_du of the exact rows of du', and those differ from the exact rows of du64
         by at most sum_i tau_du[d, i] |W[d, i, j]|; the bound as specified adds tau_W to |W| there (looser), which we keep:
         tau_rows = rows_bound(|du64| + tau_du) + sum_i tau_du[d, i] (|W[d, i, j]| + tau_W[d, i, j]).
  gS/gO  the ordered scatter adds the m_e device rows that name entity e by fp32 adds in a fixed order; the rows are
         within tau_rows of rows64, so in magnitude at most |rows64| + tau_rows:
         tau_g[e] = sum_{d -> e} tau_rows[d] + acc(m_e, sum_{d -> e} (|rows64[d]| + tau_rows[d])).
  gG     one fp32 chain over the B queries of the products (du'[d, i] * S[h_d, j]) * O[t_d, k]; the two roundings per term
         and the B - 1 adds stay within acc(B, .):
         tau_gG = sum_d (tau_du[d, i] + (B + 2) 2^-24 |du64[d, i]|) |S[h_d, j]| |O[t_d, k]|.
  bf16   gradients returned in bf16: + 2^-8 (|g64| + tau) for the rounding of the returned value.
  sym    the symmetric model's gE = gS + gO, one more add of the two returned gradients by autograd, in their type:
         fp32 + acc(2, T), bf16 + 2^-8 T, with T = |gS| + tau_gS + |gO| + tau_gO.
"""
import numpy as np

import relation_model as rm

EPS = 2.0 ** -24


def acc(n, total):
    """The fp32 accumulation bound of n terms with magnitudes adding up to ``total``."""
    return (n + 2) * EPS * total


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def pair_rows(core, X, x_idx, w):
    """rows64 (B, b) of rtk_pair_rows_f32."""
    G, Xn, wn = _f64(core, X, w)
    return np.einsum("di,ijk,dk->dj", wn, G, Xn[np.asarray(x_idx, dtype=np.int64)])


def rows_bounds(core, X, x_idx, w):
    """(rows64, tau_rows) of one rtk_pair_rows_f32 call: the forward's bound with a and b exchanged."""
    B = np.shape(w)[0]
    return rm.u_bounds(np.transpose(np.asarray(core), (1, 0, 2)), w, X, np.arange(B), x_idx, False)


def core_outer(x, y, z):
    """gG64 (a, b, c) of rtk_core_outer_f32."""
    xn, yn, zn = _f64(x, y, z)
    return np.einsum("di,dj,dk->ijk", xn, yn, zn)


def core_outer_bound(x, y, z):
    """tau of rtk_core_outer_f32 on given fp32 operands: acc(B, sum_d |x y z|)."""
    xn, yn, zn = _f64(x, y, z)
    return acc(xn.shape[0], np.einsum("di,dj,dk->ijk", np.abs(xn), np.abs(yn), np.abs(zn)))


def scatter_rows(idx, rows, n_out):
    """(out64 (n_out, n), tau) of rtk_scatter_rows_f32 on given fp32 rows; ids outside [0, n_out) add nothing."""
    idx = np.asarray(idx, dtype=np.int64)
    rn, = _f64(rows)
    ok = (idx >= 0) & (idx < n_out)
    out, mag = np.zeros((n_out, rn.shape[1])), np.zeros((n_out, rn.shape[1]))
    np.add.at(out, idx[ok], rn[ok])
    np.add.at(mag, idx[ok], np.abs(rn[ok]))
    m = np.bincount(idx[ok], minlength=n_out).astype(np.float64)[:, None]
    return out, (m + 2) * EPS * mag


def gradients(core, R, S, O, h, t, dZ):
    """The float64 gradients: dict with u, du, gR, rS, rO, gS, gO, gG."""
    G, Rn, Sn, On, dz = _f64(core, R, S, O, dZ)
    h, t = np.asarray(h, dtype=np.int64), np.asarray(t, dtype=np.int64)
    s, x = Sn[h], On[t]
    u = np.einsum("ijk,dj,dk->di", G, s, x)
    du = dz @ Rn
    rS = np.einsum("di,ijk,dk->dj", du, G, x)
    rO = np.einsum("di,ijk,dj->dk", du, G, s)
    gS, gO = np.zeros_like(Sn), np.zeros_like(On)
    np.add.at(gS, h, rS)
    np.add.at(gO, t, rO)
    return {"u": u, "du": du, "gR": dz.T @ u, "rS": rS, "rO": rO, "gS": gS, "gO": gO,
            "gG": np.einsum("di,dj,dk->ijk", du, s, x)}


def _chain_rows(core, X, x_idx, du, tau_du):
    """tau of the rows that the device sweeps from ITS du (core (a, b, c): rows over b, X (n, c))."""
    G, Xn = _f64(core, X)
    a, b, c = G.shape
    x = Xn[np.asarray(x_idx, dtype=np.int64)]
    W = np.einsum("ijk,dk->dij", G, x)
    tau_w = rm._product_bound(x, G.reshape(a * b, c), False).reshape(-1, a, b) + 2e-5 * (1.0 + np.abs(W))
    _, tau = rows_bounds(core, X, x_idx, np.abs(du) + tau_du)
    return tau + np.einsum("di,dij->dj", tau_du, np.abs(W) + tau_w)


def _chain_scatter(idx, rows, tau_rows, n_out):
    idx = np.asarray(idx, dtype=np.int64)
    tau, mag = np.zeros((n_out, rows.shape[1])), np.zeros((n_out, rows.shape[1]))
    np.add.at(tau, idx, tau_rows)
    np.add.at(mag, idx, np.abs(rows) + tau_rows)
    m = np.bincount(idx, minlength=n_out).astype(np.float64)[:, None]
    return tau + (m + 2) * EPS * mag


def grad_bounds(core, R, S, O, h, t, dZ, symmetric=False, bf16_out=False):
    """``(g64, tau)``: two dicts with the keys core, R, S, O (symmetric: core, R, E) for the end-to-end fp32 backward of
    ``relation_logits`` on the operands as given (bf16 operands: pass them rounded); ``bf16_out`` adds the rounding of
    gradients returned in bf16.  ids must lie inside their tables."""
    G, Rn, Sn, On, dz = _f64(core, R, S, O, dZ)
    h, t = np.asarray(h, dtype=np.int64), np.asarray(t, dtype=np.int64)
    B, n_rel = dz.shape
    g = gradients(core, R, S, O, h, t, dZ)
    u, tau_u = rm.u_bounds(core, S, O, h, t, bf16_out)        # the saved u is the forward's: the bf16 kernels' with bf16 operands
    du = g["du"]
    tau_du = acc(n_rel, np.abs(dz) @ np.abs(Rn))
    tau_gR = np.abs(dz).T @ tau_u + acc(B, np.abs(dz).T @ np.abs(u))
    tau_rS = _chain_rows(G, On, t, du, tau_du)
    tau_rO = _chain_rows(np.transpose(G, (0, 2, 1)), Sn, h, du, tau_du)
    tau_gS = _chain_scatter(h, g["rS"], tau_rS, Sn.shape[0])
    tau_gO = _chain_scatter(t, g["rO"], tau_rO, On.shape[0])
    tau_gG = np.einsum("di,dj,dk->ijk", tau_du + (B + 2) * EPS * np.abs(du), np.abs(Sn[h]), np.abs(On[t]))
    val = {"core": g["gG"], "R": g["gR"], "S": g["gS"], "O": g["gO"]}
    tau = {"core": tau_gG, "R": tau_gR, "S": tau_gS, "O": tau_gO}
    if bf16_out:
        tau = {k: v + 2.0 ** -8 * (np.abs(val[k]) + v) for k, v in tau.items()}
    if symmetric:
        mag = np.abs(val["S"]) + tau["S"] + np.abs(val["O"]) + tau["O"]
        val["E"], tau["E"] = val["S"] + val["O"], tau["S"] + tau["O"] + (2.0 ** -8 * mag if bf16_out else acc(2, mag))
        for k in ("S", "O"):
            del val[k], tau[k]
    return val, tau


def rows_case(a, b, c, B, seed=0, n_x=None):
    """The inputs of the rtk_pair_rows_f32 tests: a float32 core, X with power-of-two row scales, w and ids with repeats."""
    rng = np.random.default_rng(7919 * seed + 31 * a + 17 * b + c + B)
    n_x = n_x or max(2, B // 2 + 1)
    core = rng.standard_normal((a, b, c)).astype(np.float32)
    X = rm.scaled((n_x, c), seed + 1, -3, 3)
    w = rm.scaled((B, a), seed + 2, -3, 3)
    return core, X, rng.integers(0, n_x, B).astype(np.int64), w


def grad_case(a=5, b=36, n_rel=11, n_ent=60, B=70, seed=0):
    """The inputs of the end-to-end gradient tests: float32 parameters, B queries with repeated h and t, a random dZ."""
    rng = np.random.default_rng(104729 * seed + a + b + n_rel + B)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    ids = lambda: rng.integers(0, max(2, n_ent // 3), B).astype(np.int64) * 3 % n_ent
    return {"core": f(a, b, b) * np.float32(0.5), "R": f(n_rel, a), "S": f(n_ent, b), "O": f(n_ent, b), "h": ids(), "t": ids(),
            "dZ": f(B, n_rel), "rel": rng.integers(0, n_rel, B).astype(np.int64)}
