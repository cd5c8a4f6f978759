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
//   finish_kernel   partials of the slots and of the filter waves added in a fixed order; base + count written.
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

constexpr int RP_WAVES = 4;                    // waves per workgroup of the counting kernel: 128 entity rows per tile
constexpr int RP_TILE = 32 * RP_WAVES;
constexpr int RP_SLOTS = 2 * RTK_N_CU;         // rows of partials: the resident workgroups, two per CU
constexpr int RP_UQ = 8;                       // filter waves per query
constexpr int RP_MAX_KS_F32 = RTK_CG_MAX_KS;   // the ws kernel's range: c <= 208
constexpr int RP_MAX_KS_BF16 = 32;             // score_bf16_kernel's range: c <= 512

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
    typedef typename AFrag<T>::type AT;
    const int d = blockIdx.x, lane = threadIdx.x, h = lane >> 5;
    const int64_t t_raw = obj_idx[d];
    if ((t_raw < 0 || t_raw >= n_ent) && lane == 0) atomicOr(err, 4u);
    const int jl = clamp_target(t_raw, n_ent) - col0;
    if (jl < 0 || jl >= n_local) {                                   // wave-uniform: another block's object
        if (lane == 0) pt_out[d] = -INFINITY;
        return;
    }
    const int mt = d >> 5, row = d & 31;
    AT A0[KS], A1[KS];
    load_a<T, KS>(qp, mt, row, h, A0, A1);
    const float srow = Frag<T, KS>::PLANES == 2
                           ? reinterpret_cast<const float *>(qp + mt * tile_bytes<T, KS>())[row] : 1.0f;
    Frag<T, KS> f;
    f.load(O, jl, c, h, vec);
    f.template convert<SG>();
    const f32x16 acc = f.chain(A0, A1);
    if (lane == 0) pt_out[d] = f.template prob<SG>(acc[0], srow);     // element 0 of lane 0: row 0, column 0
}

// Sum of v[0 .. 15] over the 32 lanes of a half wave.  Each step trades half of the live values with lane ^ O_ and
// keeps the other half, so 8 + 4 + 2 + 1 exchanges and one last full one do the work of 16 x 5.  Afterwards lane r
// holds the total of element red_elem(r); the order of the additions is fixed.
template <int N, int O_, typename V>
__device__ __forceinline__ void reduce_step(V (&v)[16], int r) {
    const bool up = (r & O_) != 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const V send = up ? v[i] : v[i + N];
        const V keep = up ? v[i + N] : v[i];
        v[i] = keep + __shfl_xor(send, O_);
    }
}
template <typename V>
__device__ __forceinline__ V reduce16(V (&v)[16], int r) {
    reduce_step<8, 16>(v, r);
    reduce_step<4, 8>(v, r);
    reduce_step<2, 4>(v, r);
    reduce_step<1, 2>(v, r);
    return v[0] + __shfl_xor(v[0], 1);
}
__device__ __forceinline__ int red_elem(int r) { return (r >> 1) & 15; }   // bits 4..1 of r, most significant first

template <typename T, int KS>
struct CountLds {
    static constexpr int TILE = (int)tile_bytes<T, KS>();
    static constexpr int PT = TILE;                 // 32 floats: pt of the tile's rows
    static constexpr int TG = TILE + 128;           // 32 ints: clamped target ids
    static constexpr int BUF = TILE + 256;
    static constexpr int RED = 2 * BUF;             // [2][RP_WAVES][32] int counts, then the same of float BCE sums
    static constexpr int RED_BUF = RP_WAVES * 32 * 4;
    static constexpr int TOTAL = RED + 4 * RED_BUF;
};

// Step 2, dense part.  Workgroup (slot, qs): entity tiles slot, slot + n_slots, ...; query tiles of range qs.
template <typename T, int KS, int SG, bool BCE>
__global__ __launch_bounds__(64 * RP_WAVES, 2) void count_kernel(const unsigned char *__restrict__ qp, int B,
                                                                 const T *__restrict__ O, int n_local, int c, int col0,
                                                                 int n_ent, const int64_t *__restrict__ obj_idx,
                                                                 const float *__restrict__ pt_in, int n_slots, int qsplit,
                                                                 int32_t *__restrict__ part_cnt,
                                                                 float *__restrict__ part_bce, bool vec) {
    typedef typename AFrag<T>::type AT;
    typedef CountLds<T, KS> L;
    constexpr int NT = 64 * RP_WAVES;
    constexpr int CHUNKS = L::TILE / 16;
    constexpr int NLD = (CHUNKS + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int slot = (int)blockIdx.x / qsplit, qs = (int)blockIdx.x % qsplit;
    const int n_mt = (B + 31) >> 5, n_tiles = (n_local + RP_TILE - 1) / RP_TILE;
    const int mt0 = (int)((int64_t)n_mt * qs / qsplit), nq = (int)((int64_t)n_mt * (qs + 1) / qsplit) - mt0;
    if (nq <= 0 || slot >= n_tiles) return;                       // (never with the host's grid)

    u32x4 stg[NLD];
    float stg_pt = 0.f;
    auto stage_load = [&](int mt) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(qp + (int64_t)mt * L::TILE);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ch = i * NT + t;
            if (i + 1 < NLD || ch < CHUNKS) stg[i] = src[ch];
        }
        if (t < 64) {                                              // rows past the batch read the last query's values
            const int d = min(mt * 32 + (t & 31), B - 1);
            stg_pt = t < 32 ? pt_in[d] : __int_as_float(clamp_target(obj_idx[d], n_ent));
        }
    };
    auto stage_store = [&](int buf) {
        u32x4 *dst = reinterpret_cast<u32x4 *>(lds + buf * L::BUF);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ch = i * NT + t;
            if (i + 1 < NLD || ch < CHUNKS) dst[ch] = stg[i];
        }
        if (t < 64) reinterpret_cast<float *>(lds + buf * L::BUF + L::PT)[t] = stg_pt;   // PT and TG are adjacent
    };

    stage_load(mt0);
    int it = 0;                                                    // tiles staged so far: buffer parity
    bool first = true;                                             // the workgroup's first entity tile writes its partials
    for (int tile = slot; tile < n_tiles; tile += n_slots, first = false) {
        const int jl = tile * RP_TILE + wave * 32 + r;             // this lane's row of the block
        const bool valid = jl < n_local;
        const int jg = col0 + jl;
        Frag<T, KS> f;
        f.load(O, min(jl, n_local - 1), c, h, vec);
        f.template convert<SG>();
        if (tile == slot) {
            stage_store(0);
            __syncthreads();
        }
        for (int i = 0; i < nq; ++i, ++it) {
            const int cur = it & 1;
            const bool more = i + 1 < nq || tile + n_slots < n_tiles;
            if (more) stage_load(i + 1 < nq ? mt0 + i + 1 : mt0);
            const unsigned char *buf = lds + cur * L::BUF;
            const AT *la = reinterpret_cast<const AT *>(buf + RTK_PACK_HDR);
            const f32x16 acc = f.chain_with([&](int plane, int ks) { return la[(plane * KS + ks) * 64 + lane]; });
            // element e of the accumulator: query row 8 (e / 4) + 4 h + e % 4 of the tile, entity r of the wave
            int cnt[16];
            float bce[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int rw = 8 * g + 4 * h;
                const f32x4 pt4 = *reinterpret_cast<const f32x4 *>(buf + L::PT + rw * 4);
                const u32x4 tg4 = *reinterpret_cast<const u32x4 *>(buf + L::TG + rw * 4);
                f32x4 sr4 = {1.f, 1.f, 1.f, 1.f};
                if (Frag<T, KS>::PLANES == 2) sr4 = *reinterpret_cast<const f32x4 *>(buf + rw * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = 4 * g + q;
                    const float p = f.template prob<SG>(acc[e], sr4[q]);
                    const int k = (p > pt4[q]) + ((p == pt4[q]) & (jg < (int)tg4[q]));
                    cnt[e] = valid ? k : 0;
                    bce[e] = (BCE && valid) ? rtk_clog(1.0f - p) : 0.f;
                }
            }
            const int csum = reduce16(cnt, r);
            float bsum = 0.f;
            if (BCE) bsum = reduce16(bce, r);
            if (!(r & 1)) {
                const int e = red_elem(r), rw = 8 * (e >> 2) + 4 * h + (e & 3);
                reinterpret_cast<int *>(lds + L::RED + cur * L::RED_BUF)[wave * 32 + rw] = csum;
                if (BCE) reinterpret_cast<float *>(lds + L::RED + (2 + cur) * L::RED_BUF)[wave * 32 + rw] = bsum;
            }
            if (more) stage_store(cur ^ 1);
            __syncthreads();
            // query tile i of the range always belongs to wave i % RP_WAVES: its partials are read and written by
            // one wave, in tile order
            if (wave == (i & (RP_WAVES - 1)) && (BCE || h == 0)) {
                const int d = (mt0 + i) * 32 + r;
                if (d < B) {
                    const int64_t at = (int64_t)slot * B + d;
                    if (h == 0) {
                        const int *rc = reinterpret_cast<const int *>(lds + L::RED + cur * L::RED_BUF);
                        const int s = rc[r] + rc[32 + r] + rc[64 + r] + rc[96 + r];
                        part_cnt[at] = first ? s : part_cnt[at] + s;
                    } else {
                        const float *rb = reinterpret_cast<const float *>(lds + L::RED + (2 + cur) * L::RED_BUF);
                        const float s = ((rb[r] + rb[32 + r]) + rb[64 + r]) + rb[96 + r];
                        part_bce[at] = first ? s : part_bce[at] + s;
                    }
                }
            }
        }
    }
}

// Step 2, the filter correction: wave u of query d scores the CSR entries [i0 + 32 (u + RP_UQ k), + 32) of the query,
// one per column, and corrects the count for those inside the block (filtered_rank_kernel's rule, global ids).
template <typename T, int KS, int SG>
__global__ __launch_bounds__(64 * RP_WAVES) void filter_kernel(const unsigned char *__restrict__ qp, int B,
                                                               const T *__restrict__ O, int n_local, int c, int col0,
                                                               int n_ent, const int64_t *__restrict__ obj_idx,
                                                               const float *__restrict__ pt_in,
                                                               const int64_t *__restrict__ pair_slot,
                                                               const int64_t *__restrict__ pair_ptr,
                                                               const int64_t *__restrict__ pair_obj,
                                                               int32_t *__restrict__ fc_cnt, float *__restrict__ fc_bce,
                                                               bool want_bce, bool vec) {
    typedef typename AFrag<T>::type AT;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane((int)blockIdx.x * RP_WAVES + (int)(threadIdx.x >> 6));
    const int d = w / RP_UQ, u = w % RP_UQ;
    if (d >= B) return;
    int cnt = 0;
    float bce = 0.f;
    const int64_t s = pair_slot[d];
    if (s >= 0) {
        const int64_t i0 = pair_ptr[s] + 32 * u, i1 = pair_ptr[s + 1];
        if (i0 < i1) {
            const int mt = d >> 5, row = d & 31;
            AT A0[KS], A1[KS];
            load_a<T, KS>(qp, mt, row, h, A0, A1);
            const float srow = Frag<T, KS>::PLANES == 2
                                   ? reinterpret_cast<const float *>(qp + mt * tile_bytes<T, KS>())[row] : 1.0f;
            const float pt = pt_in[d];
            const int tgt = clamp_target(obj_idx[d], n_ent);
            Frag<T, KS> f;
            for (int64_t base = i0; base < i1; base += 32 * RP_UQ) {    // wave-uniform
                const int64_t i = base + r;
                const int64_t jr = i < i1 ? pair_obj[i] : -1;
                const bool ok = jr >= col0 && jr < (int64_t)col0 + n_local;
                if (__ballot(ok) == 0) continue;                       // every entry is another block's
                f.load(O, ok ? (int64_t)(jr - col0) : 0, c, h, vec);
                f.template convert<SG>();
                const f32x16 acc = f.chain(A0, A1);
                if (h == 0 && ok) {                                    // element 0 of lane r: row 0, column r
                    const float p = f.template prob<SG>(acc[0], srow);
                    if (want_bce) bce += rtk_clog(p) - rtk_clog(1.0f - p);
                    if (jr != tgt) {
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
        bce += __shfl_xor(bce, o);
    }
    if (lane == 0) {
        fc_cnt[(int64_t)d * RP_UQ + u] = cnt;
        fc_bce[(int64_t)d * RP_UQ + u] = bce;
    }
}

// counts_out[d] = base + partials of the slots + the filter waves' corrections (base 0: a block's count; base 1: the
// whole range's rank); bce_rows_out[d] = -(the same of the BCE sums).
// 32 queries per workgroup, 8 threads per query take the slots 8 apart; everything is added in a fixed order.
__global__ __launch_bounds__(256) void finish_kernel(int B, int n_slots, int col0, int n_local, int n_ent, int base,
                                                     const int32_t *__restrict__ part_cnt,
                                                     const float *__restrict__ part_bce,
                                                     const int32_t *__restrict__ fc_cnt, const float *__restrict__ fc_bce,
                                                     const int64_t *__restrict__ obj_idx,
                                                     const int64_t *__restrict__ pair_slot,
                                                     const float *__restrict__ pt_in, int32_t *__restrict__ counts_out,
                                                     double *__restrict__ bce_rows_out) {
    __shared__ int s_cnt[8][32];
    __shared__ double s_bce[8][32];
    const int t = threadIdx.x, q = t & 31, sl = t >> 5;
    const int d = min((int)blockIdx.x * 32 + q, B - 1);
    const bool want_bce = bce_rows_out != nullptr;
    int cnt = 0;
    double bce = 0.0;
    for (int k = sl; k < n_slots; k += 8) {
        cnt += part_cnt[(int64_t)k * B + d];
        if (want_bce) bce += (double)part_bce[(int64_t)k * B + d];
    }
    s_cnt[sl][q] = cnt;
    s_bce[sl][q] = bce;
    __syncthreads();
    if (sl != 0 || (int)blockIdx.x * 32 + q >= B) return;
    cnt = 0;
    bce = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        cnt += s_cnt[k][q];
        bce += s_bce[k][q];
    }
    const bool listed = pair_slot && pair_slot[d] >= 0;
    if (listed) {
#pragma unroll
        for (int u = 0; u < RP_UQ; ++u) {
            cnt += fc_cnt[(int64_t)d * RP_UQ + u];
            if (want_bce) bce += (double)fc_bce[(int64_t)d * RP_UQ + u];
        }
    } else if (want_bce) {                                   // no filter list: the queried object is the only positive
        const int jl = clamp_target(obj_idx[d], n_ent) - col0;
        const float pt = pt_in[d];
        if (jl >= 0 && jl < n_local) bce += (double)(rtk_clog(pt) - rtk_clog(1.0f - pt));
    }
    counts_out[d] = base + cnt;
    if (want_bce) bce_rows_out[d] = -bce;
}

// workgroup slots and query ranges of the counting kernel: whole entity tiles per slot; with fewer tiles than slots
// the query tiles are cut into ranges (each range converts the tile's rows again) until the slots are used
struct CountGrid {
    int n_slots, qsplit;
};
CountGrid grid_of(int64_t batch, int64_t n_local) {
    const int64_t n_tiles = rtk_cdiv(n_local, RP_TILE), n_mt = rtk_cdiv(batch, 32);
    CountGrid g;
    g.n_slots = (int)(n_tiles < RP_SLOTS ? n_tiles : RP_SLOTS);
    int64_t q = RP_SLOTS / (g.n_slots > 0 ? g.n_slots : 1);
    if (q > n_mt) q = n_mt;
    g.qsplit = (int)(q < 1 ? 1 : q);
    return g;
}

struct PartLayout {
    size_t cnt, bce, fcnt, fbce, total;
};
PartLayout layout_of(int64_t batch, int64_t n_local) {
    PartLayout L;
    const size_t slots = (size_t)grid_of(batch, n_local).n_slots;
    L.cnt = 256;                                              // [0, 256): the error word's header
    L.bce = L.cnt + rtk_align_up(slots * (size_t)batch * 4, 256);
    L.fcnt = L.bce + rtk_align_up(slots * (size_t)batch * 4, 256);
    L.fbce = L.fcnt + rtk_align_up((size_t)RP_UQ * (size_t)batch * 4, 256);
    L.total = L.fbce + rtk_align_up((size_t)RP_UQ * (size_t)batch * 4, 256);
    return L;
}

template <typename T, int KS, int SG, bool BCE>
int launch_count(const unsigned char *qp, int B, const T *O, int n_local, int c, int col0, int n_ent,
                 const int64_t *obj_idx, const float *pt, const CountGrid &g, int32_t *pcnt, float *pbce, bool vec,
                 hipStream_t st, const char *fn) {
    constexpr int bytes = CountLds<T, KS>::TOTAL;
    static std::atomic<unsigned long long> lds_ok{0};
    if (bytes > 64 * 1024) {
        const int rc = rtk_ensure_dynamic_lds(reinterpret_cast<const void *>(&count_kernel<T, KS, SG, BCE>), bytes, lds_ok, fn);
        if (rc != RTK_OK) return rc;
    }
    RTK_LAUNCH_SCORE((count_kernel<T, KS, SG, BCE>), dim3((unsigned)(g.n_slots * g.qsplit)), dim3(64 * RP_WAVES), bytes, st,
                     qp, B, O, n_local, c, col0, n_ent, obj_idx, pt, g.n_slots, g.qsplit, pcnt, pbce, vec);
    return RTK_OK;
}

// whether O's rows can be read 16 bytes at a time (bf16: a fragment is then wholly inside or outside a row)
template <typename T>
bool vec_rows(const T *O, int c) { return sizeof(T) == 4 || (c % 8 == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0); }

// Step 1 on the stream: pt_out[d] for the B queries; the error word is the workspace's first word.
template <typename T, int KS, int SG>
int launch_targets(const unsigned char *qp, int B, const T *O, int n_local, int c, int col0, int n_ent,
                   const int64_t *obj_idx, float *pt_out, unsigned char *ws, hipStream_t st) {
    hipLaunchKernelGGL((target_kernel<T, KS, SG>), dim3((unsigned)B), dim3(64), 0, st, qp, B, O, n_local, c, col0, n_ent,
                       obj_idx, pt_out, reinterpret_cast<uint32_t *>(ws), vec_rows(O, c));
    return RTK_OK;
}

// Step 2 on the stream: count_kernel, filter_kernel when there is a filter, finish_kernel writing base + count.
template <typename T, int KS, int SG>
int launch_counts(const unsigned char *qp, int B, const T *O, int n_local, int c, int col0, int n_ent, const float *pt,
                  const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                  int base, int32_t *counts, double *bce_rows, unsigned char *ws, hipStream_t st, const char *fn) {
    const PartLayout L = layout_of(B, n_local);
    const CountGrid g = grid_of(B, n_local);
    int32_t *pcnt = reinterpret_cast<int32_t *>(ws + L.cnt);
    float *pbce = reinterpret_cast<float *>(ws + L.bce);
    int32_t *fcnt = reinterpret_cast<int32_t *>(ws + L.fcnt);
    float *fbce = reinterpret_cast<float *>(ws + L.fbce);
    const bool vec = vec_rows(O, c);
    const int rc = bce_rows ? launch_count<T, KS, SG, true>(qp, B, O, n_local, c, col0, n_ent, obj_idx, pt, g, pcnt, pbce, vec, st, fn)
                            : launch_count<T, KS, SG, false>(qp, B, O, n_local, c, col0, n_ent, obj_idx, pt, g, pcnt, pbce, vec, st, fn);
    if (rc != RTK_OK) return rc;
    if (pair_slot)
        hipLaunchKernelGGL((filter_kernel<T, KS, SG>), dim3((unsigned)rtk_cdiv((int64_t)B * RP_UQ, RP_WAVES)),
                           dim3(64 * RP_WAVES), 0, st, qp, B, O, n_local, c, col0, n_ent, obj_idx, pt, pair_slot, pair_ptr,
                           pair_obj, fcnt, fbce, bce_rows != nullptr, vec);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)rtk_cdiv(B, 32)), dim3(256), 0, st, B, g.n_slots, col0, n_local, n_ent,
                       base, pcnt, pbce, fcnt, fbce, obj_idx, pair_slot, pt, counts, bce_rows);
    return RTK_OK;
}

// f(K, SG) instantiated for the k-steps of c and the logistic the flags select, then the launch check
template <typename T, typename F>
int dispatch(const char *fn, int c, unsigned flags, F f) {
    const bool fast = (flags & RTK_SCORE_SIGMOID_FAST) != 0;
    const int rc = rtk_dispatch_ksteps<sizeof(T) == 4 ? RP_MAX_KS_F32 : RP_MAX_KS_BF16>((c + 15) / 16, fn, [&](auto K) {
        return fast ? f(K, std::integral_constant<int, 2>{}) : f(K, std::integral_constant<int, 1>{});
    });
    return rc != RTK_OK ? rc : rtk_check_launch(fn);
}

// the checks every entry point shares; `out` is the call's output, `ws_extra` what it keeps behind the block layout
template <typename T>
int check_block(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
                int64_t n_ent, const int64_t *obj_idx, unsigned flags, const void *out, const void *workspace,
                size_t ws_bytes, size_t ws_extra = 0) {
    constexpr bool F32 = sizeof(T) == 4;
    RTK_REQUIRE(q_packed && O && obj_idx && out && workspace, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(batch >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld must be >= 0", fn, (long long)batch);
    RTK_REQUIRE(n_ent >= 1, RTK_ERR_BAD_ARG, "%s: n_ent = %lld must be >= 1", fn, (long long)n_ent);
    RTK_REQUIRE(col0 >= 0 && n_local >= 1 && n_local <= n_ent && col0 <= n_ent - n_local, RTK_ERR_BAD_ARG,
                "%s: block col0 = %lld, n_local = %lld is not a non-empty part of [0, n_ent = %lld)", fn, (long long)col0,
                (long long)n_local, (long long)n_ent);
    RTK_REQUIRE(c >= 1, RTK_ERR_BAD_ARG, "%s: object rank c = %d must be >= 1", fn, c);
    RTK_REQUIRE(batch < (1ll << 31) - 32 && n_ent < (1ll << 31) - 64, RTK_ERR_UNSUPPORTED, "%s: dimension too large", fn);
    RTK_REQUIRE(flags & RTK_SCORE_SIGMOID, RTK_ERR_UNSUPPORTED,
                "%s: ranks are taken on probabilities: flags need RTK_SCORE_SIGMOID (raw logits are not ranked)", fn);
    RTK_REQUIRE((flags & ~(RTK_SCORE_SIGMOID | RTK_SCORE_SIGMOID_FAST)) == 0, RTK_ERR_BAD_ARG, "%s: unknown flags 0x%x",
                fn, flags);
    if (F32) {
        RTK_REQUIRE(c <= 16 * RP_MAX_KS_F32, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d (the ws kernel's range)", fn, c,
                    16 * RP_MAX_KS_F32);
        RTK_REQUIRE(c % 4 == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0, RTK_ERR_UNSUPPORTED,
                    "%s: fp32 needs c %% 4 == 0 and a 16-byte-aligned O (c = %d)", fn, c);
    } else {
        RTK_REQUIRE(c <= 16 * RP_MAX_KS_BF16, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d", fn, c, 16 * RP_MAX_KS_BF16);
    }
    const size_t need = layout_of(batch, n_local).total + ws_extra;
    RTK_REQUIRE(ws_bytes >= need, RTK_ERR_BAD_ARG, "%s: workspace of %zu bytes given, %zu needed", fn, ws_bytes, need);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_BAD_ARG, "%s: workspace must be 256-byte aligned",
                fn);
    return RTK_OK;
}

template <typename T>
int rank_targets(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
                 int64_t n_ent, const int64_t *obj_idx, unsigned flags, float *pt_out, void *workspace, size_t ws_bytes,
                 void *stream) {
    const int rc = check_block<T>(fn, q_packed, batch, c, O, n_local, col0, n_ent, obj_idx, flags, pt_out, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        return launch_targets<T, K.value, SG.value>((const unsigned char *)q_packed, (int)batch, O, (int)n_local, c, (int)col0,
                                                    (int)n_ent, obj_idx, pt_out, (unsigned char *)workspace,
                                                    (hipStream_t)stream);
    });
}

template <typename T>
int rank_counts(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
                int64_t n_ent, const float *pt, const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                const int64_t *pair_obj, unsigned flags, int32_t *counts_out, double *bce_rows_out, void *workspace,
                size_t ws_bytes, void *stream) {
    RTK_REQUIRE(pt, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", fn);
    const int rc = check_block<T>(fn, q_packed, batch, c, O, n_local, col0, n_ent, obj_idx, flags, counts_out, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        return launch_counts<T, K.value, SG.value>((const unsigned char *)q_packed, (int)batch, O, (int)n_local, c, (int)col0,
                                                   (int)n_ent, pt, obj_idx, pair_slot, pair_ptr, pair_obj, 0, counts_out,
                                                   bce_rows_out, (unsigned char *)workspace, (hipStream_t)stream, fn);
    });
}

// The whole range as one block: both steps at col0 = 0, n_local = n_ent, pt behind the block layout, ranks = 1 + count.
template <typename T>
int score_rank(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_ent,
               const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
               unsigned flags, int32_t *ranks, double *bce_rows, void *workspace, size_t ws_bytes, void *stream) {
    RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", fn);
    const int rc = check_block<T>(fn, q_packed, batch, c, O, n_ent, 0, n_ent, obj_idx, flags, ranks, workspace, ws_bytes,
                                  rtk_align_up((size_t)(batch > 0 ? batch : 0) * 4, 256));
    if (rc != RTK_OK || batch == 0) return rc;
    unsigned char *ws = (unsigned char *)workspace;
    float *pt = reinterpret_cast<float *>(ws + layout_of(batch, n_ent).total);
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        const unsigned char *qp = (const unsigned char *)q_packed;
        const int B = (int)batch, N = (int)n_ent;
        hipStream_t st = (hipStream_t)stream;
        launch_targets<T, K.value, SG.value>(qp, B, O, N, c, 0, N, obj_idx, pt, ws, st);
        return launch_counts<T, K.value, SG.value>(qp, B, O, N, c, 0, N, pt, obj_idx, pair_slot, pair_ptr, pair_obj, 1, ranks,
                                                   bce_rows, ws, st, fn);
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
    return rank_counts<float>("rtk_score_rank_counts_f32", q_packed, batch, c, O_local, n_local, col0, n_ent, pt, obj_idx,
                              pair_slot, pair_ptr, pair_obj, flags, counts_out, bce_rows_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_score_rank_counts_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                          int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                                          const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                          unsigned flags, int32_t *counts_out, double *bce_rows_out, void *workspace,
                                          size_t ws_bytes, void *stream) {
    return rank_counts<rtk_bf16>("rtk_score_rank_counts_bf16", q_packed, batch, c, (const rtk_bf16 *)O_local, n_local, col0,
                                 n_ent, pt, obj_idx, pair_slot, pair_ptr, pair_obj, flags, counts_out, bce_rows_out,
                                 workspace, ws_bytes, stream);
}
