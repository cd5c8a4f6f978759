// The ordered scatter (rtk_scatter.hip; internal header): gO[e, :] = sum over the entries i with entity e of
// dz[i] v[query of i, :], for M entries, with no float atomics.  The one way a gradient reaches the rows of the entity
// matrix from a list of (entity, query) pairs: rtk_score_candidates_bwd_*, rtk_bce_stream_grad_o*_f32, rtk_ce_stream_grad_f32.
//
// THE ORDER OF THE SUMS (it decides the bits of gO; tests/golden/scatter_cases.py emulates it):
//   * an entity outside [0, n_ent) becomes the key n_ent, sorts last and adds nothing;
//   * the entries are sorted by entity with a stable sort: increasing i within an entity (a run);
//   * window w owns the sorted positions [w win, (w + 1) win); inside a window every run starts from 0 and adds
//     fmaf(dz[i], v[d, col], acc) in sorted order, each column on its own;
//   * a run inside one window is stored as it is; a run over several windows is the partial sum of the window where it
//     starts plus the partial sums of the following windows, in window order, by plain fp32 adds;
//   * a row of gO that no entry names is zero: gO is zeroed first, then written.
// So the bits depend on the entries and on `win` alone.  The two front ends choose `win`:
//   candidates   win = rtk_scatter_window(M), M = batch x K exact: short windows fill the chip on small problems;
//   flat lists   win = RTK_SCATTER_WIN_MAX always: there m is the caller's BOUND on the entries (the surplus slots carry
//                an invalid entity), and the bits must not depend on a bound.
#pragma once
#include "rtk_common.h"

constexpr int RTK_SCATTER_WIN_MAX = 256;      // most sorted entries per wave of the run sum
constexpr int RTK_SCATTER_MAXC = 1024;        // longest row (c) the run sum holds in registers

// Entries per wave of the run sum: M / 4096 (a quarter of a wave's share at 16 waves per CU), 16 to RTK_SCATTER_WIN_MAX.
// A wave walks its window in a chain of dependent loads, so small problems need short windows to fill the chip.
static inline int64_t rtk_scatter_window(int64_t M) {
    const int64_t w = rtk_cdiv(rtk_cdiv(M, 4096), 16) * 16;
    return w < 16 ? 16 : (w > RTK_SCATTER_WIN_MAX ? RTK_SCATTER_WIN_MAX : w);
}

// Workspace bytes for M entries (0 for M <= 0), 256-byte aligned pieces: the partial sums are sized for the shortest
// window a front end may use at this M, rtk_scatter_window(M).
size_t rtk_scatter_bytes(int64_t M);

// The (batch, k) candidate matrix: entry i = d k + j has entity cand[d ld_cand + j], query d and dz[d ld_dz + j].
int rtk_scatter_candidates(const char *fn, const int64_t *cand, int64_t ld_cand, int64_t batch, int64_t k, int64_t n_ent,
                           const float *dz, int64_t ld_dz, const float *v, int c, float *gO, void *workspace, hipStream_t st);

// Flat lists: entry i < m has entity ent[i], query owner[i] and dz[i].
int rtk_scatter_flat(const char *fn, const int32_t *ent, const int32_t *owner, const float *dz, int64_t m, int64_t n_ent,
                     const float *v, int c, float *gO, void *workspace, hipStream_t st);

// The same with a row pitch on v: query d's row starts at v + d ld_v (ld_v >= c).  The sums are those of ld_v == c.
int rtk_scatter_flat_ld(const char *fn, const int32_t *ent, const int32_t *owner, const float *dz, int64_t m, int64_t n_ent,
                        const float *v, int64_t ld_v, int c, float *gO, void *workspace, hipStream_t st);
