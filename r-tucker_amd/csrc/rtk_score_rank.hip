// Filtered ranks of (h, r, t) queries without the score matrix: against every entity (rtk_score_rank_*) and on one
// block of entity rows (rtk_score_rank_targets_* / rtk_score_rank_counts_*, the matrix-free form of
// rtk_target_scores_f32 / rtk_filtered_rank_partial_f32, rtk_rank.hip).
//
//   rank_d = 1 + #{ j : p'_j > p_t } + #{ j < t : p'_j == p_t }       (the rule of rtk_filtered_rank_f32, rtk_rank.hip)
//
// p'_j is p_j with the query's other known-true objects replaced by 0; among equal probabilities the lower entity id
// ranks first.  A rank of a process group holds rows [col0, col0 + n_local) of O:
//
//   step 1  rtk_score_rank_targets_*   pt[d] = p(d, t_d) where the block owns t_d, -inf elsewhere      (all-reduce MAX)
//   step 2  rtk_score_rank_counts_*    the block's share of #{j : p'_j > pt} + #{j < t : p'_j == pt}    (all-reduce SUM)
//
// rtk_score_rank_* is the one-block call: both steps at col0 = 0, n_local = n_ent, pt kept in the workspace and the
// finish pass writing 1 + count.  There is one set of kernels.
//
// Step 2 has three modes (Stable, StableBce, Ties below), chosen at compile time by the entry point.  The stable modes
// give the count above, StableBce with the rows' BCE sums; rtk_score_rank_tie_counts_* is the Ties mode: the two counts
// of the tie-aware ranks in place of their stable combination,
//
//   greater = #{ j != t : p'_j > pt }      equal = #{ j != t : p'_j == pt }      (1 + greater <= rank <= 1 + greater + equal)
//
// Every mode keeps two planes of partials: int32 counts, and a second plane whose element type the mode names -- float
// BCE sums or int32 `equal` counts.
//
// Step 1 is target_kernel: one wave per query, p_t from a 32x32 MFMA tile whose rows are all query d and whose column 0
// is O[t_d].  Step 2 is three launches on the caller's stream:
//
//   count_kernel    entity-stationary.  A workgroup of 4 waves takes 128 consecutive rows of O; each wave converts its 32
//                   rows into B fragments ONCE, keeps them in registers and sweeps the query tiles, whose packed A
//                   planes the workgroup stages through a double-buffered LDS tile (with the tile's pt and target ids).
//                   The 32 x 32 probabilities are compared with pt and counted, never stored.  A lane holds one entity and
//                   16 query rows: the 16 counts (and BCE terms) are summed over the 32 entity lanes by a halving
//                   butterfly (16 exchanges instead of 80), over the 4 waves in wave order, and added to the
//                   workgroup's own row of partials -- always by the same wave, in tile order.  The grid is persistent:
//                   at most RP_SLOTS workgroup slots (two per CU) walk the entity tiles; with fewer tiles than slots the
//                   query tiles are cut into ranges so that the chip stays full.
//   filter_kernel   RP_UQ waves per query: wave u re-scores the query's CSR entries [32 (u + RP_UQ k), +32) that fall in
//                   the block and takes them out of (or keeps them in) the count as filtered_rank_kernel does.
//   finish_kernel   partials of the slots and of the filter waves added in a fixed order; base + count written, and
//                   the second plane's sum (-BCE row sum, or `equal`) by the modes that have one.
//
// Exactness.  Every probability comes from Frag<T, KS> (rtk_score_rank_kernel.h).  A score's bits depend only on its
// query row, its entity row and c: an MFMA output element does not depend on its position in the tile, the O row
// conversion is per row, and the row factors come from the packed header.  The element arithmetic is that of the stored
// kernels -- fp32: the O row scaling and hi/lo split of the ws kernel (rtk_score_ws_kernel.h, m_role), one chain of 3
// MFMAs per k-step in the order hi*hi, hi*lo, lo*hi, then acc * (row factor * column factor) and the logistic the flags
// select; bf16: score_bf16_kernel's chain(s) and logistic.  Keep Frag in step with those kernels (tests/test_gpu_rank.py
// compares with them bit for bit).  Integer counts are exact whatever the order, so the counts of any partition of
// [0, n_ent) add up to the whole range's; the BCE sums are float partials reduced in the fixed order above (no float
// atomics), so repeated calls give the same bits.
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_rank_kernel.h"
#include "rtk_score_select.h"

namespace {

constexpr int RP_WAVES = SW_WAVES;             // the counting kernel is a sweep: 128 entity rows per tile
constexpr int RP_SLOTS = SW_SLOTS;             // rows of partials: the resident workgroups, two per CU
constexpr int RP_UQ = 8;                       // filter waves per query

// The modes of step 2.  second_t: what the second plane of partials holds (of the slots and of the filter waves);
// sum_t: what the finish pass adds them up in and writes out.
struct Stable {                                // base + #{p' > pt} + #{j < t : p' == pt}
    typedef float second_t;                    // (unused)
    typedef double sum_t;
    static constexpr bool BCE = false, TIES = false;
};
struct StableBce {                             // the same, and the rows' BCE sums
    typedef float second_t;                    // float BCE partials
    typedef double sum_t;
    static constexpr bool BCE = true, TIES = false;
};
struct Ties {                                  // greater = #{j != t : p' > pt} and equal = #{j != t : p' == pt}
    typedef int32_t second_t;                  // `equal` counts
    typedef int32_t sum_t;
    static constexpr bool BCE = false, TIES = true;
};
// the stable mode a call's bce_rows selects
template <typename F>
int stable_mode(const double *bce_rows, F f) {
    return bce_rows ? f(StableBce{}) : f(Stable{});
}

// the queried object's id as every kernel here sees it: clamped into [0, n_ent) (an id outside sets bit 2 of the error
// word in target_kernel)
__device__ __forceinline__ int clamp_target(int64_t t, int n_ent) { return (int)(t < 0 ? 0 : (t >= n_ent ? n_ent - 1 : t)); }

// Step 1: one wave per query; a 32 x 32 tile whose rows are all query d and whose column 0 is O[t_d - col0]; a block
// that does not own t_d writes -inf.
template <typename T, int KS, int SG>
__global__ __launch_bounds__(64) void target_kernel(const unsigned char *__restrict__ qp, int B, const T *__restrict__ O,
                                                    int n_local, int c, int col0, int n_ent,
                                                    const int64_t *__restrict__ obj_idx, float *__restrict__ pt_out,
                                                    uint32_t *__restrict__ err, bool vec) {
    const int d = blockIdx.x, lane = threadIdx.x, h = lane >> 5;
    const int64_t t_raw = obj_idx[d];
    if ((t_raw < 0 || t_raw >= n_ent) && lane == 0) atomicOr(err, 4u);
    const int jl = clamp_target(t_raw, n_ent) - col0;
    if (jl < 0 || jl >= n_local) {                                   // wave-uniform: another block's object
        if (lane == 0) pt_out[d] = -INFINITY;
        return;
    }
    QueryRow<T, KS> q;
    q.load(qp, d, h);
    Frag<T, KS> f;
    const float p = q.template score<SG>(f, O, jl, c, h, vec);
    if (lane == 0) pt_out[d] = p;                                    // element 0 of lane 0: row 0, column 0
}

// LDS of the counting kernel: two query tiles, each with its rows' pt and target ids behind it, then the waves' sums
template <typename T, int KS>
struct CountLds {
    static constexpr int TILE = (int)tile_bytes<T, KS>();
    static constexpr int EXTRA = 256;               // 32 floats: pt of the tile's rows; 32 ints: clamped target ids
    static constexpr int PT = TILE;
    static constexpr int TG = TILE + 128;
    static constexpr int BUF = TILE + EXTRA;
    static constexpr int RED = 2 * BUF;             // [2][RP_WAVES][32] int counts, then the same of float BCE sums
    static constexpr int RED_BUF = RP_WAVES * 32 * 4;
    static constexpr int TOTAL = RED + 4 * RED_BUF;
};

// What count_kernel does with the sweep (rtk_score_rank_kernel.h).  The 32 x 32 probabilities are compared with pt and
// counted, never stored.  A lane holds one entity and 16 query rows: the 16 counts (and BCE terms) are summed over the
// 32 entity lanes by the butterfly, over the 4 waves in wave order, and added to the workgroup's own row of partials.
//
// Ties: the two counts of the tie-aware ranks instead (rtk_score_rank_tie_counts_*): an element contributes p > pt and
// (p == pt) & (j != t).  A 32-lane sum of either is at most 32 and the sum over the 4 waves at most 128, so both travel
// as one int (greater | equal << 16) through the butterfly and the LDS slot -- the exchanges and the LDS of the plain
// count -- and publish unpacks them into the mode's two int32 planes (totals reach n_local): greater into part_cnt,
// equal into part_second.
template <typename T, int KS, int SG, typename Mode>
struct CountSweep {
    static constexpr bool BCE = Mode::BCE, TIES = Mode::TIES;
    typedef CountLds<T, KS> L;
    static constexpr int EXTRA = L::EXTRA;
    int B, col0, n_ent;
    const int64_t *__restrict__ obj_idx;
    const float *__restrict__ pt_in;
    int32_t *__restrict__ part_cnt;
    typename Mode::second_t *__restrict__ part_second;
    float stg_pt = 0.f;

    __device__ __forceinline__ void load_extra(SweepLane ln, int mt) {
        const int t = ln.t;
        if (t < 64) {                                              // rows past the batch read the last query's values
            const int d = min(mt * 32 + (t & 31), B - 1);
            stg_pt = t < 32 ? pt_in[d] : __int_as_float(clamp_target(obj_idx[d], n_ent));
        }
    }
    __device__ __forceinline__ void store_extra(SweepLane ln, int extra) const {
        if (ln.t < 64) reinterpret_cast<float *>(sweep_lds + extra)[ln.t] = stg_pt;  // PT and TG are adjacent
    }
    __device__ __forceinline__ void begin_tile() const {}
    __device__ __forceinline__ void end_tile(SweepLane, int) const {}
    __device__ __forceinline__ void score(SweepLane ln, const Frag<T, KS> &f, const f32x16 &acc,
                                          const unsigned char *buf, int cur, int jl, bool valid, int) const {
        const int wave = ln.wave, r = ln.r, h = ln.h;
        const int jg = col0 + jl;
        int cnt[16];
        float bce[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rw = acc_row(4 * g, h);
            const f32x4 pt4 = *reinterpret_cast<const f32x4 *>(buf + L::PT + rw * 4);
            const u32x4 tg4 = *reinterpret_cast<const u32x4 *>(buf + L::TG + rw * 4);
            f32x4 sr4 = {1.f, 1.f, 1.f, 1.f};
            if (Frag<T, KS>::PLANES == 2) sr4 = *reinterpret_cast<const f32x4 *>(buf + rw * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                const float p = f.template prob<SG>(acc[e], sr4[q]);
                const int k = TIES ? (p > pt4[q]) | (((p == pt4[q]) & (jg != (int)tg4[q])) << 16)
                                   : (p > pt4[q]) + ((p == pt4[q]) & (jg < (int)tg4[q]));
                cnt[e] = valid ? k : 0;
                bce[e] = (BCE && valid) ? rtk_clog(1.0f - p) : 0.f;
            }
        }
        const int csum = reduce16(cnt, r, RedSum());
        float bsum = 0.f;
        if (BCE) bsum = reduce16(bce, r, RedSum());
        if (!(r & 1)) {
            const int rw = red_row(r, h);
            reinterpret_cast<int *>(sweep_lds + L::RED + cur * L::RED_BUF)[wave * 32 + rw] = csum;
            if (BCE) reinterpret_cast<float *>(sweep_lds + L::RED + (2 + cur) * L::RED_BUF)[wave * 32 + rw] = bsum;
        }
    }
    // query tile i of the range always belongs to wave i % RP_WAVES: its partials are read and written by one wave, in
    // tile order; the workgroup's first entity tile writes them
    __device__ __forceinline__ void publish(SweepLane ln, int cur, int i, int mt, int slot, int, bool first) const {
        const int wave = ln.wave, r = ln.r, h = ln.h;
        if (wave == (i & (RP_WAVES - 1)) && (BCE || TIES || h == 0)) {
            const int d = mt * 32 + r;
            if (d < B) {
                const int64_t at = (int64_t)slot * B + d;
                if constexpr (TIES) {                              // half 0: greater, half 1: equal
                    const int *rc = reinterpret_cast<const int *>(sweep_lds + L::RED + cur * L::RED_BUF);
                    const int both = rc[r] + rc[32 + r] + rc[64 + r] + rc[96 + r];
                    const int s = h == 0 ? (both & 0xffff) : (both >> 16);
                    int32_t *plane = h == 0 ? part_cnt : part_second;
                    plane[at] = first ? s : plane[at] + s;
                } else if (h == 0) {
                    const int *rc = reinterpret_cast<const int *>(sweep_lds + L::RED + cur * L::RED_BUF);
                    const int s = rc[r] + rc[32 + r] + rc[64 + r] + rc[96 + r];
                    part_cnt[at] = first ? s : part_cnt[at] + s;
                } else {
                    const float *rb = reinterpret_cast<const float *>(sweep_lds + L::RED + (2 + cur) * L::RED_BUF);
                    const float s = ((rb[r] + rb[32 + r]) + rb[64 + r]) + rb[96 + r];
                    part_second[at] = first ? s : part_second[at] + s;
                }
            }
        }
    }
};

// Step 2, dense part.  Workgroup (slot, qs): entity tiles slot, slot + n_slots, ...; query tiles of range qs.
template <typename T, int KS, int SG, typename Mode>
__global__ __launch_bounds__(64 * RP_WAVES, 2) void count_kernel(const unsigned char *__restrict__ qp, int B,
                                                                 const T *__restrict__ O, int n_local, int c, int col0,
                                                                 int n_ent, const int64_t *__restrict__ obj_idx,
                                                                 const float *__restrict__ pt_in, int n_slots, int qsplit,
                                                                 int32_t *__restrict__ part_cnt,
                                                                 typename Mode::second_t *__restrict__ part_second,
                                                                 bool vec) {
    CountSweep<T, KS, SG, Mode> pol{B, col0, n_ent, obj_idx, pt_in, part_cnt, part_second};
    sweep<T, KS, SG>(pol, qp, B, O, n_local, c, vec, n_slots, qsplit);
}

// Step 2, the filter correction: wave u of query d scores the CSR entries [i0 + 32 (u + RP_UQ k), + 32) of the query,
// one per column, and corrects the count for those inside the block (filtered_rank_kernel's rule, global ids).
// The correction depends on the mode only through what the second plane holds.  float (the stable modes): the entries'
// BCE terms when want_bce.  int32 (Ties): the corrections of the two tie counts -- the entry leaves `greater` or `equal`
// and, now a 0, joins `equal` when the target score is 0 -- in fc_cnt (greater) and fc_second (equal).
template <typename T, int KS, int SG, typename Second>
__global__ __launch_bounds__(64 * RP_WAVES) void filter_kernel(const unsigned char *__restrict__ qp, int B,
                                                               const T *__restrict__ O, int n_local, int c, int col0,
                                                               int n_ent, const int64_t *__restrict__ obj_idx,
                                                               const float *__restrict__ pt_in,
                                                               const int64_t *__restrict__ pair_slot,
                                                               const int64_t *__restrict__ pair_ptr,
                                                               const int64_t *__restrict__ pair_obj,
                                                               int32_t *__restrict__ fc_cnt,
                                                               Second *__restrict__ fc_second, bool want_bce, bool vec) {
    constexpr bool TIES = std::is_same<Second, int32_t>::value;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane((int)blockIdx.x * RP_WAVES + (int)(threadIdx.x >> 6));
    const int d = w / RP_UQ, u = w % RP_UQ;
    if (d >= B) return;
    int cnt = 0, eq = 0;
    float bce = 0.f;
    const int64_t s = pair_slot[d];
    if (s >= 0) {
        const int64_t i0 = pair_ptr[s] + 32 * u, i1 = pair_ptr[s + 1];
        if (i0 < i1) {
            QueryRow<T, KS> q;
            q.load(qp, d, h);
            const float pt = pt_in[d];
            const int tgt = clamp_target(obj_idx[d], n_ent);
            Frag<T, KS> f;
            for (int64_t base = i0; base < i1; base += 32 * RP_UQ) {    // wave-uniform
                const int64_t i = base + r;
                const int64_t jr = i < i1 ? pair_obj[i] : -1;
                const bool ok = jr >= col0 && jr < (int64_t)col0 + n_local;
                if (__ballot(ok) == 0) continue;                       // every entry is another block's
                const float p = q.template score<SG>(f, O, ok ? (int64_t)(jr - col0) : 0, c, h, vec);
                if (h == 0 && ok) {                                    // element 0 of lane r: row 0, column r
                    if (want_bce) bce += rtk_clog(p) - rtk_clog(1.0f - p);
                    if (TIES) {
                        if (jr != tgt) {
                            cnt -= p > pt;
                            eq -= p == pt;
                            eq += 0.0f == pt;                 // now a 0: ties only with a zero target score
                        }
                    } else if (jr != tgt) {
                        cnt -= p > pt;
                        cnt -= (p == pt) & (jr < tgt);
                        cnt += (0.0f == pt) & (jr < tgt);     // now a 0: ties only with a zero target score
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        if (TIES) eq += __shfl_xor(eq, o);
        else bce += __shfl_xor(bce, o);
    }
    if (lane == 0) {
        fc_cnt[(int64_t)d * RP_UQ + u] = cnt;
        if constexpr (TIES) fc_second[(int64_t)d * RP_UQ + u] = eq;
        else fc_second[(int64_t)d * RP_UQ + u] = bce;
    }
}

// counts_out[d] = base + partials of the slots + the filter waves' corrections (base 0: a block's count; base 1: the
// whole range's rank); second_out[d] = the same of the second plane, by the modes that have one: StableBce -(the BCE
// sums), floats added as doubles; Ties the `equal` counts.
// 32 queries per workgroup, 8 threads per query take the slots 8 apart; everything is added in a fixed order.
template <typename Mode>
__global__ __launch_bounds__(256) void finish_kernel(int B, int n_slots, int col0, int n_local, int n_ent, int base,
                                                     const int32_t *__restrict__ part_cnt,
                                                     const typename Mode::second_t *__restrict__ part_second,
                                                     const int32_t *__restrict__ fc_cnt,
                                                     const typename Mode::second_t *__restrict__ fc_second,
                                                     const int64_t *__restrict__ obj_idx,
                                                     const int64_t *__restrict__ pair_slot,
                                                     const float *__restrict__ pt_in, int32_t *__restrict__ counts_out,
                                                     typename Mode::sum_t *__restrict__ second_out) {
    typedef typename Mode::sum_t sum_t;
    constexpr bool SECOND = Mode::BCE || Mode::TIES;
    __shared__ int s_cnt[8][32];
    __shared__ sum_t s_sec[8][32];
    const int t = threadIdx.x, q = t & 31, sl = t >> 5;
    const int d = min((int)blockIdx.x * 32 + q, B - 1);
    int cnt = 0;
    sum_t sec = 0;
    for (int k = sl; k < n_slots; k += 8) {
        cnt += part_cnt[(int64_t)k * B + d];
        if (SECOND) sec += (sum_t)part_second[(int64_t)k * B + d];
    }
    s_cnt[sl][q] = cnt;
    if (SECOND) s_sec[sl][q] = sec;
    __syncthreads();
    if (sl != 0 || (int)blockIdx.x * 32 + q >= B) return;
    cnt = 0;
    sec = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        cnt += s_cnt[k][q];
        if (SECOND) sec += s_sec[k][q];
    }
    if (pair_slot && pair_slot[d] >= 0) {
#pragma unroll
        for (int u = 0; u < RP_UQ; ++u) {
            cnt += fc_cnt[(int64_t)d * RP_UQ + u];
            if (SECOND) sec += (sum_t)fc_second[(int64_t)d * RP_UQ + u];
        }
    } else if (Mode::BCE) {                                  // no filter list: the queried object is the only positive
        const int jl = clamp_target(obj_idx[d], n_ent) - col0;
        const float pt = pt_in[d];
        if (jl >= 0 && jl < n_local) sec += (sum_t)(rtk_clog(pt) - rtk_clog(1.0f - pt));
    }
    counts_out[d] = base + cnt;
    if (SECOND) second_out[d] = Mode::BCE ? -sec : sec;
}

struct PartLayout {
    size_t cnt, bce, fcnt, fbce, total;
};
PartLayout layout_of(int64_t batch, int64_t n_local) {
    PartLayout L;
    const size_t slots = (size_t)grid_of(batch, n_local, RP_SLOTS).n_slots;
    L.cnt = 256;                                              // [0, 256): the error word's header
    L.bce = L.cnt + rtk_align_up(slots * (size_t)batch * 4, 256);
    L.fcnt = L.bce + rtk_align_up(slots * (size_t)batch * 4, 256);
    L.fbce = L.fcnt + rtk_align_up((size_t)RP_UQ * (size_t)batch * 4, 256);
    L.total = L.fbce + rtk_align_up((size_t)RP_UQ * (size_t)batch * 4, 256);
    return L;
}

// Step 1 on the stream: pt_out[d] for the B queries; the error word is the workspace's first word.
template <typename T, int KS, int SG>
int launch_targets(const unsigned char *qp, int B, const T *O, int n_local, int c, int col0, int n_ent,
                   const int64_t *obj_idx, float *pt_out, unsigned char *ws, hipStream_t st) {
    hipLaunchKernelGGL((target_kernel<T, KS, SG>), dim3((unsigned)B), dim3(64), 0, st, qp, B, O, n_local, c, col0, n_ent,
                       obj_idx, pt_out, reinterpret_cast<uint32_t *>(ws), vec_rows(O, c));
    return RTK_OK;
}

// Step 2 on the stream: count_kernel, filter_kernel when there is a filter, finish_kernel writing base + count and the
// mode's second output.  The second planes get the mode's element type here, once.
template <typename T, int KS, int SG, typename Mode>
int launch_counts(const unsigned char *qp, int B, const T *O, int n_local, int c, int col0, int n_ent, const float *pt,
                  const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                  int base, int32_t *counts, typename Mode::sum_t *second_out, unsigned char *ws, hipStream_t st,
                  const char *fn) {
    typedef typename Mode::second_t second_t;
    const PartLayout L = layout_of(B, n_local);
    const SweepGrid g = grid_of(B, n_local, RP_SLOTS);
    int32_t *pcnt = reinterpret_cast<int32_t *>(ws + L.cnt);
    second_t *psec = reinterpret_cast<second_t *>(ws + L.bce);
    int32_t *fcnt = reinterpret_cast<int32_t *>(ws + L.fcnt);
    second_t *fsec = reinterpret_cast<second_t *>(ws + L.fbce);
    const bool vec = vec_rows(O, c);
    const int rc = launch_lds<&count_kernel<T, KS, SG, Mode>, CountLds<T, KS>::TOTAL>(
        dim3((unsigned)(g.n_slots * g.qsplit)), dim3(64 * RP_WAVES), st, fn, qp, B, O, n_local, c, col0, n_ent, obj_idx, pt,
        g.n_slots, g.qsplit, pcnt, psec, vec);
    if (rc != RTK_OK) return rc;
    if (pair_slot)
        hipLaunchKernelGGL((filter_kernel<T, KS, SG, second_t>), dim3((unsigned)rtk_cdiv((int64_t)B * RP_UQ, RP_WAVES)),
                           dim3(64 * RP_WAVES), 0, st, qp, B, O, n_local, c, col0, n_ent, obj_idx, pt, pair_slot, pair_ptr,
                           pair_obj, fcnt, fsec, Mode::BCE, vec);
    hipLaunchKernelGGL(finish_kernel<Mode>, dim3((unsigned)rtk_cdiv(B, 32)), dim3(256), 0, st, B, g.n_slots, col0, n_local,
                       n_ent, base, pcnt, psec, fcnt, fsec, obj_idx, pair_slot, pt, counts, second_out);
    return RTK_OK;
}

// the checks every entry point shares; `out` is the call's output, `ws_extra` what it keeps behind the block layout
template <typename T>
int check_rank(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
               int64_t n_ent, const int64_t *obj_idx, unsigned flags, const void *out, const void *workspace,
               size_t ws_bytes, size_t ws_extra = 0) {
    return check_block(fn, q_packed && obj_idx && out, batch, c, O, n_local, col0, n_ent, [] { return (int)RTK_OK; },
                       (1ll << 31) - 64, flags, "ranks are", workspace, ws_bytes, [&] { return layout_of(batch, n_local).total + ws_extra; });
}

template <typename T>
int rank_targets(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
                 int64_t n_ent, const int64_t *obj_idx, unsigned flags, float *pt_out, void *workspace, size_t ws_bytes,
                 void *stream) {
    const int rc = check_rank<T>(fn, q_packed, batch, c, O, n_local, col0, n_ent, obj_idx, flags, pt_out, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        return launch_targets<T, K.value, SG.value>((const unsigned char *)q_packed, (int)batch, O, (int)n_local, c, (int)col0,
                                                    (int)n_ent, obj_idx, pt_out, (unsigned char *)workspace,
                                                    (hipStream_t)stream);
    });
}

// Step 2 of a block in one mode.  Stable: second_out is unused; StableBce: the BCE row sums; Ties: counts_out is
// `greater`, second_out `equal`, and both are required.
template <typename T, typename Mode>
int rank_counts(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
                int64_t n_ent, const float *pt, const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                const int64_t *pair_obj, unsigned flags, int32_t *counts_out, typename Mode::sum_t *second_out,
                void *workspace, size_t ws_bytes, void *stream) {
    RTK_REQUIRE(pt, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", fn);
    const int rc = check_rank<T>(fn, q_packed, batch, c, O, n_local, col0, n_ent, obj_idx, flags,
                                  Mode::TIES && !second_out ? nullptr : counts_out, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        return launch_counts<T, K.value, SG.value, Mode>((const unsigned char *)q_packed, (int)batch, O, (int)n_local, c,
                                                         (int)col0, (int)n_ent, pt, obj_idx, pair_slot, pair_ptr, pair_obj,
                                                         0, counts_out, second_out, (unsigned char *)workspace,
                                                         (hipStream_t)stream, fn);
    });
}

// The whole range as one block: both steps at col0 = 0, n_local = n_ent, pt behind the block layout, ranks = 1 + count.
template <typename T>
int score_rank(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_ent,
               const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
               unsigned flags, int32_t *ranks, double *bce_rows, void *workspace, size_t ws_bytes, void *stream) {
    RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", fn);
    const int rc = check_rank<T>(fn, q_packed, batch, c, O, n_ent, 0, n_ent, obj_idx, flags, ranks, workspace, ws_bytes,
                                  rtk_align_up((size_t)(batch > 0 ? batch : 0) * 4, 256));
    if (rc != RTK_OK || batch == 0) return rc;
    unsigned char *ws = (unsigned char *)workspace;
    float *pt = reinterpret_cast<float *>(ws + layout_of(batch, n_ent).total);
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        const unsigned char *qp = (const unsigned char *)q_packed;
        const int B = (int)batch, N = (int)n_ent;
        hipStream_t st = (hipStream_t)stream;
        launch_targets<T, K.value, SG.value>(qp, B, O, N, c, 0, N, obj_idx, pt, ws, st);
        return stable_mode(bce_rows, [&](auto mode) {
            return launch_counts<T, K.value, SG.value, decltype(mode)>(qp, B, O, N, c, 0, N, pt, obj_idx, pair_slot, pair_ptr,
                                                                       pair_obj, 1, ranks, bce_rows, ws, st, fn);
        });
    });
}

}  // namespace

// the block layout at n_local = n_ent, and B floats of pt behind it
extern "C" size_t rtk_score_rank_workspace_bytes(int dtype, int64_t batch, int64_t n_ent, int c) {
    (void)dtype;
    (void)c;
    if (batch < 0 || n_ent < 1) return 0;
    return layout_of(batch, n_ent).total + rtk_align_up((size_t)batch * 4, 256);
}

extern "C" int rtk_score_rank_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_ent,
                                  const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                                  const int64_t *pair_obj, unsigned flags, int32_t *ranks, double *bce_rows,
                                  void *workspace, size_t ws_bytes, void *stream) {
    return score_rank<float>("rtk_score_rank_f32", q_packed, batch, c, O, n_ent, obj_idx, pair_slot, pair_ptr, pair_obj,
                             flags, ranks, bce_rows, workspace, ws_bytes, stream);
}

extern "C" int rtk_score_rank_bf16(const void *q_packed, int64_t batch, int c, const void *O, int64_t n_ent,
                                   const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                                   const int64_t *pair_obj, unsigned flags, int32_t *ranks, double *bce_rows,
                                   void *workspace, size_t ws_bytes, void *stream) {
    return score_rank<rtk_bf16>("rtk_score_rank_bf16", q_packed, batch, c, (const rtk_bf16 *)O, n_ent, obj_idx, pair_slot, pair_ptr,
                                pair_obj, flags, ranks, bce_rows, workspace, ws_bytes, stream);
}

extern "C" size_t rtk_score_rank_part_workspace_bytes(int dtype, int64_t batch, int64_t n_local, int c) {
    (void)dtype;
    (void)c;
    if (batch < 0 || n_local < 1) return 0;
    return layout_of(batch, n_local).total;
}

extern "C" int rtk_score_rank_targets_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                          int64_t col0, int64_t n_ent, const int64_t *obj_idx, unsigned flags,
                                          float *pt_out, void *workspace, size_t ws_bytes, void *stream) {
    return rank_targets<float>("rtk_score_rank_targets_f32", q_packed, batch, c, O_local, n_local, col0, n_ent, obj_idx,
                               flags, pt_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_score_rank_targets_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                           int64_t col0, int64_t n_ent, const int64_t *obj_idx, unsigned flags,
                                           float *pt_out, void *workspace, size_t ws_bytes, void *stream) {
    return rank_targets<rtk_bf16>("rtk_score_rank_targets_bf16", q_packed, batch, c, (const rtk_bf16 *)O_local, n_local,
                                  col0, n_ent, obj_idx, flags, pt_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_score_rank_counts_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                         int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                                         const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                         unsigned flags, int32_t *counts_out, double *bce_rows_out, void *workspace,
                                         size_t ws_bytes, void *stream) {
    return stable_mode(bce_rows_out, [&](auto mode) {
        return rank_counts<float, decltype(mode)>("rtk_score_rank_counts_f32", q_packed, batch, c, O_local, n_local, col0,
                                                  n_ent, pt, obj_idx, pair_slot, pair_ptr, pair_obj, flags, counts_out,
                                                  bce_rows_out, workspace, ws_bytes, stream);
    });
}

extern "C" int rtk_score_rank_counts_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                          int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                                          const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                          unsigned flags, int32_t *counts_out, double *bce_rows_out, void *workspace,
                                          size_t ws_bytes, void *stream) {
    return stable_mode(bce_rows_out, [&](auto mode) {
        return rank_counts<rtk_bf16, decltype(mode)>("rtk_score_rank_counts_bf16", q_packed, batch, c,
                                                     (const rtk_bf16 *)O_local, n_local, col0, n_ent, pt, obj_idx, pair_slot,
                                                     pair_ptr, pair_obj, flags, counts_out, bce_rows_out, workspace, ws_bytes,
                                                     stream);
    });
}

// the block layout (the Ties mode's second planes hold the equal counts); 0 outside the covered range
extern "C" size_t rtk_score_rank_ties_workspace_bytes(int dtype, int64_t batch, int64_t n_local, int c) {
    if (batch < 0 || batch >= (1ll << 31) - 32 || n_local < 1 || n_local >= (1ll << 31) - 64 || c < 1) return 0;
    if (dtype == RTK_F32 ? (c > 16 * SW_MAX_KS_F32 || c % 4 != 0) : (dtype != RTK_BF16 || c > 16 * SW_MAX_KS_BF16)) return 0;
    return layout_of(batch, n_local).total;
}

extern "C" int rtk_score_rank_tie_counts_f32(const void *q_packed, int64_t batch, int c, const float *O_local,
                                             int64_t n_local, int64_t col0, int64_t n_ent, const float *pt,
                                             const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                                             const int64_t *pair_obj, unsigned flags, int32_t *greater_out,
                                             int32_t *equal_out, void *workspace, size_t ws_bytes, void *stream) {
    return rank_counts<float, Ties>("rtk_score_rank_tie_counts_f32", q_packed, batch, c, O_local, n_local, col0, n_ent, pt,
                                    obj_idx, pair_slot, pair_ptr, pair_obj, flags, greater_out, equal_out, workspace,
                                    ws_bytes, stream);
}

extern "C" int rtk_score_rank_tie_counts_bf16(const void *q_packed, int64_t batch, int c, const void *O_local,
                                              int64_t n_local, int64_t col0, int64_t n_ent, const float *pt,
                                              const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                                              const int64_t *pair_obj, unsigned flags, int32_t *greater_out,
                                              int32_t *equal_out, void *workspace, size_t ws_bytes, void *stream) {
    return rank_counts<rtk_bf16, Ties>("rtk_score_rank_tie_counts_bf16", q_packed, batch, c, (const rtk_bf16 *)O_local,
                                       n_local, col0, n_ent, pt, obj_idx, pair_slot, pair_ptr, pair_obj, flags, greater_out,
                                       equal_out, workspace, ws_bytes, stream);
}
