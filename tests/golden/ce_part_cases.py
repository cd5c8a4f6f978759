"""Cases, float64 references and bounds for the block form of the matrix-free cross-entropy kernels
(rtk_ce_stream_rows_part_f32 / rtk_ce_stream_grad_part_f32): ce_kernel_cases.stream_forward's terms restricted to the
rows [col0, col0 + n_local) of the entity matrix, from the same constants (U, ARG) and the same model of the chain.

What a block's forward gives, and what it is held to (per query d, j over the block's columns only):

  m        the largest logit.  Family E's logits are exact in fp32, so m is float32(max_j z_j) bit for bit.  Family G: the
           device takes the maximum of logits that are each within chain_bound dz_j of z_j, so
               z_j* - dz_j*  <=  m  <=  max_j (z_j + dz_j),      j* the maximising column of the reference.
  m + ln s the block's own log-sum-exp, formed by the test in float64 from the float m and the float64 s.  The bound is
           stream_forward's dl with H, the softmax p and the chain term taken over the block, one rescale per tile of a
           split with the split edges of n_local tiles (the sweep cuts the BLOCK's tiles), and no |lse| u term (no
           float32 lse is stored):  (ARG H_b + 19 + 2 R_b) u + 1.01 sum_j p_j dz_j + 2^-50 (1 + |lse_b|).
  lin      -t0 sum_j z_j - coef_d sum_{t in P_d, t in block} z_t with t0 = eps / n_ent -- the GLOBAL entity count -- and
           coef_d = (1 - eps) / n_d from the GLOBAL stored list length: stream_forward's rows bound without its w dl
           part, sums over the block:
               t0 (16 u sum|z_j| + sum dz_j) + coef ((ceil(n_d / 128) + 10) u sum|z_t| + sum dz_t)
                   + 2^-50 (t0 sum|z_j| + coef sum|z_t|)
           (the positives' chain runs over the whole list, so its length term keeps n_d).

The merged lse M + ln sum_k s_k exp(m_k - M) is a float64 computation on the blocks' results: since
lse = ln sum_k exp(lse_k), its error is at most the largest block error, plus 2^-50 (1 + |lse|).

The backward is judged by ce_kernel_cases.stream_backward_verdict on the dv shares summed (in fp32, block order) and gO
concatenated against the whole-matrix reference, at twice its bound: the order of the fp32 sums over the blocks
differs from the whole-matrix sweep's, and the power of two of the dv product is the block's own.

Mutants (host proof, tests/test_ce_part_cases_host.py): t0 = eps / n_local, n_d = the block's count, a merge without the
maxima.  Each must leave its bound by a factor of ten or more on MUTANT_CASE (n_ent = 64 in two blocks of 32,
eps = 0.5, max |z| near 100)."""
from dataclasses import dataclass

import numpy as np

import ce_kernel_cases as cc

U, ARG = cc.U, cc.ARG


@dataclass(frozen=True)
class PartCase:
    """A StreamCase and the cuts of [0, N) into blocks."""
    case: cc.StreamCase
    cuts: tuple

    @property
    def name(self):
        return self.case.name + "_cuts" + "_".join(str(x) for x in self.cuts[1:-1])

    @property
    def blocks(self):
        return [(a, b - a) for a, b in zip(self.cuts[:-1], self.cuts[1:])]


def _stream_case(family, B, N, c, sigma=3.0):
    hit = [s for s in cc.STREAM_CASES if (s.family, s.B, s.N, s.c, s.sigma) == (family, B, N, c, sigma)]
    assert len(hit) == 1, (family, B, N, c, sigma)
    return hit[0]


# No cut is a multiple of 32.  Query 0's dominant logit sits in the last row, so the last block holds it and no other
# does.  (0, 1) of N = 95 and (1001, 1) of N = 4099 are blocks of one row; (2, 31) of N = 33 has 31 rows.
B1_CASE = cc.StreamCase("G", 1, 95, 20, lengths=(1,))         # B = 1: 256 splits for the one tile of a 31-row block
PART_CASES = [
    PartCase(_stream_case("E", 33, 95, 20), (0, 1, 45, 95)),
    PartCase(_stream_case("G", 33, 95, 20), (0, 1, 45, 95)),
    PartCase(_stream_case("E", 70, 4099, 100), (0, 1001, 1002, 4099)),
    PartCase(_stream_case("G", 70, 4099, 100), (0, 1001, 1002, 4099)),
    PartCase(_stream_case("E", 70, 3003, 208), (0, 1501, 3003)),
    PartCase(_stream_case("G", 70, 3003, 208), (0, 1501, 3003)),
    PartCase(_stream_case("G", 31, 33, 4, sigma=25.0), (0, 2, 33)),
    PartCase(B1_CASE, (0, 31, 62, 95)),
]
MUTANT_CASE = PartCase(cc.StreamCase("G", 33, 64, 20, eps=0.5, sigma=25.0), (0, 32, 64))
MUTANTS = ("t0_from_n_local", "n_d_from_the_block", "merge_without_maxima")


def _block_positives(csr, d, N, col0, n_local):
    t = csr.positives(d, N)
    return t[(t >= col0) & (t < col0 + n_local)]


def block_forward(case, data, col0, n_local, mutant=None):
    """float64 references and bounds of one block: dict(m, lse, lin, m_lo, m_hi, lse_b, lin_b)."""
    B, N = case.B, case.N
    t0, dt, _ = cc.consts64(N, case.eps)                      # t0 = eps / n_ent: the GLOBAL count
    if mutant == "t0_from_n_local":
        t0 = cc.consts64(n_local, case.eps)[0]
    csr = data.csr
    z = data.z[:, col0:col0 + n_local]
    dz = cc.chain_bound(case, data)[:, col0:col0 + n_local]
    n = csr.stored().astype(np.float64)                       # the GLOBAL (stored) list length
    pos = [_block_positives(csr, d, N, col0, n_local) - col0 for d in range(B)]
    if mutant == "n_d_from_the_block":
        n = np.array([len(t) for t in pos], dtype=np.float64)
    coef = np.where(n > 0, dt / np.maximum(n, 1), 0.0)
    pz = np.array([z[d, t].sum() for d, t in enumerate(pos)])
    paz = np.array([np.abs(z[d, t]).sum() for d, t in enumerate(pos)])
    pdz = np.array([dz[d, t].sum() for d, t in enumerate(pos)])
    m, jstar = z.max(axis=1), z.argmax(axis=1)
    lse = cc.lse64(z)
    lin = -t0 * z.sum(axis=1) - coef * pz
    p = np.exp(z - lse[:, None])
    H = (p * (m[:, None] - z)).sum(axis=1)
    edges = cc.split_edges(B, n_local)                        # the sweep cuts the block's own tiles
    R = max(b - a for a, b in zip(edges[:-1], edges[1:]))
    lse_b = (ARG * H + 19 + 2 * R) * U + 1.01 * (p * dz).sum(axis=1) + 2.0 ** -50 * (1.0 + np.abs(lse))
    az = np.abs(z).sum(axis=1)
    n_glob = csr.stored()
    lin_b = t0 * (16 * U * az + dz.sum(axis=1)) + coef * ((-(-n_glob // 128) + 10) * U * paz + pdz) \
        + 2.0 ** -50 * (t0 * az + coef * paz)
    return dict(m=m, lse=lse, lin=lin, m_lo=m - dz[np.arange(B), jstar], m_hi=(z + dz).max(axis=1), lse_b=lse_b, lin_b=lin_b)


def merge_lse(ms, ss, mutant=None):
    """M + ln sum_k s_k exp(m_k - M) in float64 (the rule of ops.ce_merge_lse)."""
    m, s = np.stack([np.asarray(x, dtype=np.float64) for x in ms]), np.stack([np.asarray(x, dtype=np.float64) for x in ss])
    M = m.max(axis=0)
    f = np.ones_like(m) if mutant == "merge_without_maxima" else np.exp(m - M[None, :])
    return M + np.log((s * f).sum(axis=0))


def merged_lse_reference(pc, data):
    """(the whole rows' float64 lse, its bound for blocks merged in float64)."""
    lse = cc.lse64(data.z)
    worst = np.max([block_forward(pc.case, data, a, n)["lse_b"] for a, n in pc.blocks], axis=0)
    return lse, worst + 2.0 ** -50 * (1.0 + np.abs(lse))


def block_forward_verdict(case, ref, got_m, got_s, got_lin):
    """-> (m ok, largest error / bound of m + ln s, of lin).  got_m: float32; got_s, got_lin: float64."""
    if not (np.isfinite(got_m).all() and np.isfinite(got_s).all() and np.isfinite(got_lin).all() and (got_s > 0).all()):
        return False, np.inf, np.inf
    gm = got_m.astype(np.float64)
    if case.family == "E":
        m_ok = np.array_equal(np.ascontiguousarray(got_m, dtype=np.float32).view(np.uint32),
                              ref["m"].astype(np.float32).view(np.uint32))
    else:
        m_ok = bool(np.all(gm >= ref["m_lo"]) and np.all(gm <= ref["m_hi"]))
    r_lse = cc._ratio(np.abs(gm + np.log(got_s) - ref["lse"]), ref["lse_b"])
    return m_ok, r_lse, cc._ratio(np.abs(got_lin - ref["lin"]), ref["lin_b"])
