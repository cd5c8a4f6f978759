"""A plain numpy model of relation prediction, (h, ?, t) (test support, no GPU, no library):

    W[d, i, j] = sum_k G[i, j, k] * O[t_d, k]
    u[d, i]    = sum_j S[h_d, j] * W[d, i, j]
    z[d, r]    = sum_i u[d, i] * R[r, i]            p = 1 / (1 + exp(-z))

in float64 on the operands as stored (bf16 operands are exact in float64), the error bounds of the device path stated
from the bounds the score kernels are already tested to (tests/test_gpu_score_cg.py, tests/test_gpu_score_bf16.py),
and the filtered tie counts of the (B, n_rel) matrix with the relation id as the target column (tests/tie_model.py).

Bounds (x_d = O[t_d], s_d = S[h_d]):

    tau_W   fp32  2e-5 (1 + |W64|) + 2^-20 c max|x_d| max_k |G[i, j, :]|
            bf16  2^-23 * 16 ceil(c / 16) * sum_k |x_d[k]| |G[i, j, k]|
    tau_u   sum_j |s_d[j]| tau_W[d, i, j]  +  (b + 4) 2^-23 sum_j |s_d[j] W64[d, i, j]|
            (one rounding of each product and an fp32 sum of at most b terms in any order, with a factor two of slack)
    tau_z   sum_i |R[r, i]| tau_u[d, i]  +  the stage-2 kernel's own bound on ITS inputs, the same two formulas with a in
            the place of c.  Its inputs are the device's u, which tau_u places within |u64| + tau_u; in bf16 they are
            rounded to bf16 first: 2^-8 sum_i |u64[d, i] R[r, i]| more.
    tau_p   3e-6 + tau_z / 4
"""
import numpy as np

import tie_model


def bf16_round(x):
    """float32 values rounded to bfloat16 (nearest even), returned as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def w64(core, O, t):
    """W64 (B, a, b)."""
    G, On = _f64(core, O)
    return np.einsum("ijk,dk->dij", G, On[np.asarray(t, dtype=np.int64)])


def pair_vectors(core, S, O, h, t):
    """u64 (B, a)."""
    Sn, = _f64(S)
    return np.einsum("dij,dj->di", w64(core, O, t), Sn[np.asarray(h, dtype=np.int64)])


def logits(core, R, S, O, h, t):
    """z64 (B, n_rel): the 1-vs-all logit of (h_d, r) at column t_d."""
    Rn, = _f64(R)
    return pair_vectors(core, S, O, h, t) @ Rn.T


def probs(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def _product_bound(x, M, bf16):
    """The score kernels' bound on x (B, K) . M (N, K)^T -> (B, N), without the fp32 path's 2e-5 (1 + |z|) term."""
    K = x.shape[1]
    if bf16:
        return 2.0 ** -23 * 16 * -(-K // 16) * (np.abs(x) @ np.abs(M).T)
    return 2.0 ** -20 * K * np.abs(x).max(axis=1, initial=0.0)[:, None] * np.abs(M).max(axis=1, initial=0.0)[None, :]


def u_bounds(core, S, O, h, t, bf16):
    """(u64, tau_u), both (B, a)."""
    G, Sn, On = _f64(core, S, O)
    a, b, c = G.shape
    x, s = On[np.asarray(t, dtype=np.int64)], Sn[np.asarray(h, dtype=np.int64)]
    W = np.einsum("ijk,dk->dij", G, x)
    tau_w = _product_bound(x, G.reshape(a * b, c), bf16).reshape(-1, a, b)
    if not bf16:
        tau_w = tau_w + 2e-5 * (1.0 + np.abs(W))
    sa = np.abs(s)[:, None, :]
    u = np.einsum("dij,dj->di", W, s)
    tau_u = (sa * tau_w).sum(axis=2) + (b + 4) * 2.0 ** -23 * (sa * np.abs(W)).sum(axis=2)
    return u, tau_u


def z_bounds(core, R, S, O, h, t, bf16):
    """(z64, tau_z, tau_p), all (B, n_rel)."""
    Rn, = _f64(R)
    u, tau_u = u_bounds(core, S, O, h, t, bf16)
    z = u @ Rn.T
    tau = tau_u @ np.abs(Rn).T
    u_in = np.abs(u) + tau_u                                    # what stage 2 is given, in magnitude
    if bf16:
        u_in = u_in * (1.0 + 2.0 ** -8)
    stage2 = _product_bound(u_in, Rn, bf16)
    if bf16:
        stage2 = stage2 + 2.0 ** -8 * (np.abs(u) @ np.abs(Rn).T)
    else:
        stage2 = stage2 + 2e-5 * (1.0 + np.abs(z) + tau)
    tau_z = tau + stage2
    return z, tau_z, 3e-6 + tau_z / 4


def tie_counts(P, rel, known=None):
    """(greater, equal, before) of the (B, n_rel) float32 matrix ``P`` with the relation id as the target column and
    each query's OTHER known relations (``known``: one list per query, or None) set to 0 -- tests/tie_model.py."""
    return tie_model.tie_counts(P, rel, known)


def tie_counts_loop(P, rel, known=None):
    """The same counts by a loop over the queries and the relations (the check of ``tie_counts``)."""
    P = np.asarray(P, dtype=np.float32)
    out = np.zeros((3, P.shape[0]), dtype=np.int64)
    for d in range(P.shape[0]):
        t = int(rel[d])
        others = set() if known is None or known[d] is None else {int(g) for g in known[d]} - {t}
        for j in range(P.shape[1]):
            if j == t:
                continue
            pj = np.float32(0.0) if j in others else P[d, j]
            out[0, d] += pj > P[d, t]
            out[1, d] += pj == P[d, t]
            out[2, d] += (pj == P[d, t]) and j < t
    return out[0], out[1], out[2]


def band(p64, rel, known, tau):
    """The float64 band of the two tie counts: ``lo[d] = #{p64_j > p64_t + tau}``, ``hi[d] = #{p64_j >= p64_t - tau}`` over
    the other relations j that the filter leaves in (``tau``: one value per query).  The device's ``greater`` and
    ``greater + equal`` on scores within tau / 2 of p64 lie in [lo, hi]."""
    p64 = np.asarray(p64, dtype=np.float64)
    B, n = p64.shape
    rel = np.asarray(rel, dtype=np.int64).reshape(-1)
    keep = np.ones((B, n), dtype=bool)
    keep[np.arange(B), rel] = False
    if known is not None:
        for d, ids in enumerate(known):
            if ids is not None:
                keep[d, [g for g in ids if g != rel[d]]] = False
    pt = p64[np.arange(B), rel][:, None]
    tau = np.asarray(tau, dtype=np.float64).reshape(-1, 1)
    return ((p64 > pt + tau) & keep).sum(1), ((p64 >= pt - tau) & keep).sum(1)


def relation_lists(triples):
    """{(s, o): sorted distinct relations} of (s, r, o) id triples."""
    out = {}
    for s, r, o in np.asarray(triples, dtype=np.int64).reshape(-1, 3).tolist():
        out.setdefault((s, o), set()).add(r)
    return {k: sorted(v) for k, v in out.items()}


def scaled(shape, seed, lo=-6, hi=6):
    """Seeded normal rows with power-of-two row scales over 2^lo .. 2^hi (float32), as tests/test_gpu_score_cg.py draws
    its operands; the last axis is the row."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    return x * np.exp2(rng.integers(lo, hi + 1, size=tuple(shape[:-1]) + (1,))).astype(np.float32)


def rank_case(n_rel, B=2000, seed=0, n_ent=60):
    """The inputs of the rank tests: seeded parameters scaled so that the logits have a standard deviation near 3, B
    queries (h, r, t) and a filter with several known relations per (h, t) pair.  Returns a dict of float32 / int64
    arrays and ``known``, one list of relation ids per query (the queried one among them).

    The band of the rank tests, [#{p64_j > p64_t + tau}, #{p64_j >= p64_t - tau}] with tau twice the query's largest
    tau_p, must be tight for the test to say anything.  tau is about 1e-4 at best: tau_z holds 2e-5 (1 + |z|) of stage 2
    alone.  With Gaussian parameters at any rank the 236 competitors of a query fall within tau of the target too often
    (measured: the two ends coincide for 70 % to 83 % of the queries at n_rel = 237, 95 % to 98 % at n_rel = 22).  So the
    case is built so that a query's logits are bounded and evenly spaced: relation rank a = 1, z[d, r] = u_d R[r] with
    R a shuffled lattice on [-1, 1], and the queries drawn from the (h, t) pairs whose |u| lies within a factor 1.25 of
    the median, so that |z| stays below about 6.5 and neighbouring probabilities are further apart than tau.  The core
    carries 2^10 and S 2^-10: W is then far above 1 and the absolute part of tau_W does not count.  (What the kernels do
    at a > 1 is the subject of the other tests.)"""
    rng = np.random.default_rng(1000 * n_rel + seed)
    b = c = 4
    core = rng.standard_normal((1, b, c)).astype(np.float32)
    S = rng.standard_normal((n_ent, b)).astype(np.float32)
    O = rng.standard_normal((n_ent, c)).astype(np.float32)
    R = np.linspace(-1, 1, n_rel, dtype=np.float32)[rng.permutation(n_rel)].reshape(n_rel, 1)
    hh, tt = [x.ravel() for x in np.meshgrid(np.arange(n_ent), np.arange(n_ent), indexing="ij")]
    u = pair_vectors(core, S, O, hh, tt)[:, 0]
    med = np.median(np.abs(u))
    ok = np.nonzero((np.abs(u) > 0.8 * med) & (np.abs(u) < 1.25 * med))[0]
    core *= np.float32(3.0 / (np.sqrt((u[ok] ** 2).mean()) * R.std()))
    core, S = core * np.float32(1024), S / np.float32(1024)
    pick = ok[rng.integers(0, len(ok), B)]
    h, t = hh[pick].astype(np.int64), tt[pick].astype(np.int64)
    r = rng.integers(0, n_rel, B).astype(np.int64)
    n_known = min(4, n_rel)
    lists = {}
    for d in range(B):
        key = (int(h[d]), int(t[d]))
        if key not in lists:
            lists[key] = set(rng.choice(n_rel, size=n_known, replace=False).tolist())
        lists[key].add(int(r[d]))
    known = [sorted(lists[(int(h[d]), int(t[d]))]) for d in range(B)]
    return {"core": core, "R": R, "S": S, "O": O, "h": h, "r": r, "t": t, "known": known, "n_ent": n_ent}
