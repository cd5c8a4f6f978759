// Filtered ranks of (h, r, t) queries against every entity, without the (B, N) score matrix.
//
//   rank_d = 1 + #{ j : p'_j > p_t } + #{ j < t : p'_j == p_t }       (the rule of rtk_filtered_rank_f32, rtk_rank.hip)
//
// p'_j is p_j with the query's other known-true objects replaced by 0.  Three launches on the caller's stream:
//
//   1. pair_kernel (targets)   one wave per query: p_t from a 32x32 MFMA tile whose rows are all query d and whose
//                              column 0 is O[t_d] -> pt[d].
//   2. sweep_kernel            query-stationary waves: a wave keeps the A fragments of one 32-query tile in registers
//                              and sweeps a contiguous range of 32-entity groups, converting each group's O rows into
//                              B fragments, running the MFMA chain and comparing the 32 x 32 probabilities with its
//                              rows' p_t in registers.  Counts (and the BCE row sums) are reduced over the wave's lanes
//                              in a fixed tree and written per (entity range, row): no atomics, no score store.
//   3. pair_kernel (filter)    one wave per query: the partial counts summed, then the query's CSR entries scored 32 at
//                              a time as in 1 and taken out of the count as filtered_rank_kernel does; "+1".
//
// Exactness.  A score's bits depend only on its query row, its entity row and c: an MFMA output element does not depend
// on its position in the tile, the O row conversion is per row, and the row factors come from the packed header.  The
// element arithmetic below is that of the stored kernels -- fp32: the O row scaling and hi/lo split of the ws kernel
// (rtk_score_ws_kernel.h, m_role), one chain of 3 MFMAs per k-step in the order hi*hi, hi*lo, lo*hi, then
// acc * (row factor * column factor) and the logistic the flags select; bf16: score_bf16_kernel's chain(s) and
// logistic.  Keep them in step with those kernels (tests/test_gpu_rank.py compares with them bit for bit).
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_rank_kernel.h"
#include "rtk_score_select.h"

namespace {

constexpr int RK_WAVES = 4;          // waves per workgroup of the sweep (independent: no LDS, no barrier)
constexpr int RK_MAX_KS_F32 = RTK_CG_MAX_KS;   // the ws kernel's range: c <= 208
constexpr int RK_MAX_KS_BF16 = 32;             // score_bf16_kernel's range: c <= 512

// Per-query pass.  FILTER == false: pt[d] = p(d, t_d) (t_d clamped into [0, N) for the load; an id outside sets
// bit 2 of the error word).  FILTER == true: partial counts and BCE sums of the sweep added up, the CSR entries of
// the query taken out (filtered_rank_kernel's correction), rank and BCE written.
template <typename T, int KS, int SG, bool FILTER>
__global__ __launch_bounds__(64) void pair_kernel(const unsigned char *__restrict__ qp, int B, const T *__restrict__ O,
                                                  int N, int c, const int64_t *__restrict__ obj_idx,
                                                  const int64_t *__restrict__ pair_slot, const int64_t *__restrict__ pair_ptr,
                                                  const int64_t *__restrict__ pair_obj, float *__restrict__ pt_out,
                                                  const int32_t *__restrict__ part_cnt, const float *__restrict__ part_bce,
                                                  int n_chunks, int32_t *__restrict__ ranks, double *__restrict__ bce_rows,
                                                  uint32_t *__restrict__ err, bool vec) {
    typedef typename AFrag<T>::type AT;
    const int d = blockIdx.x, lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int mt = d >> 5, row = d & 31;
    AT A0[KS], A1[KS];
    load_a<T, KS>(qp, mt, row, h, A0, A1);
    const float srow = Frag<T, KS>::PLANES == 2
                           ? reinterpret_cast<const float *>(qp + mt * tile_bytes<T, KS>())[row] : 1.0f;
    const int64_t t_raw = obj_idx[d];
    const int64_t tgt = t_raw < 0 ? 0 : (t_raw >= N ? N - 1 : t_raw);
    Frag<T, KS> f;
    if (!FILTER) {
        if ((t_raw < 0 || t_raw >= N) && lane == 0) atomicOr(err, 4u);
        f.load(O, tgt, c, h, vec);
        f.template convert<SG>();
        const f32x16 acc = f.chain(A0, A1);
        // element 0 of lane 0: row 0 (query d), column 0 (O[t])
        if (lane == 0) pt_out[d] = f.template prob<SG>(acc[0], srow);
        return;
    }
    const float pt = pt_out[d];
    int cnt = 0;
    float bce = 0.f;
    const bool want_bce = bce_rows != nullptr;
    const int64_t s = pair_slot ? pair_slot[d] : -1;
    if (s >= 0) {
        const int64_t i0 = pair_ptr[s], i1 = pair_ptr[s + 1];
        for (int64_t base = i0; base < i1; base += 32) {      // wave-uniform: 32 entries per tile, one per column
            const int64_t i = base + r;
            const int64_t jr = i < i1 ? pair_obj[i] : -1;
            const bool ok = jr >= 0 && jr < N;
            f.load(O, ok ? jr : 0, c, h, vec);
            f.template convert<SG>();
            const f32x16 acc = f.chain(A0, A1);
            if (h == 0 && ok) {                                // element 0 of lane r: row 0, column r
                const float p = f.template prob<SG>(acc[0], srow);
                if (want_bce) bce += clog(p) - clog(1.0f - p);
                if (jr != tgt) {
                    cnt -= p > pt;
                    cnt -= (p == pt) & (jr < tgt);
                    cnt += (0.0f == pt) & (jr < tgt);     // now a 0: ties only with a zero target score
                }
            }
        }
    } else if (want_bce && lane == 0) {                  // no filter list: the queried object is the only positive
        bce += clog(pt) - clog(1.0f - pt);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        bce += __shfl_xor(bce, o);
    }
    // the sweep's partials, in range order
    int total = 0;
    double bsum = 0.0;
    for (int k = lane; k < n_chunks; k += 64) total += part_cnt[(int64_t)k * B + d];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    if (want_bce && lane == 0)
        for (int k = 0; k < n_chunks; ++k) bsum += (double)part_bce[(int64_t)k * B + d];
    if (lane == 0) {
        ranks[d] = 1 + total + cnt;
        if (want_bce) bce_rows[d] = -(bsum + (double)bce);
    }
}

// Counting sweep: wave w takes query tile w % n_mt and entity range w / n_mt (32-column groups [g0, g1)).
template <typename T, int KS, int SG, bool BCE>
__global__ __launch_bounds__(64 * RK_WAVES) void sweep_kernel(const unsigned char *__restrict__ qp, int B,
                                                              const T *__restrict__ O, int N, int c,
                                                              const int64_t *__restrict__ obj_idx,
                                                              const float *__restrict__ pt_in, int n_chunks,
                                                              int32_t *__restrict__ part_cnt, float *__restrict__ part_bce,
                                                              bool vec) {
    typedef typename AFrag<T>::type AT;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane((int)blockIdx.x * RK_WAVES + (int)(threadIdx.x >> 6));
    const int n_mt = (B + 31) >> 5;
    const int mt = w % n_mt, chunk = w / n_mt;
    if (chunk >= n_chunks) return;
    const int G = (N + 31) >> 5;
    const int g0 = (int)((int64_t)G * chunk / n_chunks), g1 = (int)((int64_t)G * (chunk + 1) / n_chunks);
    AT A0[KS], A1[KS];
    load_a<T, KS>(qp, mt, r, h, A0, A1);
    // element e of the accumulator: row 8 (e / 4) + 4 h + e % 4, column r
    float srow[16], pt[16];
    int tgt[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int rw = 8 * (e >> 2) + 4 * h + (e & 3), d = min(mt * 32 + rw, B - 1);
        srow[e] = Frag<T, KS>::PLANES == 2 ? reinterpret_cast<const float *>(qp + mt * tile_bytes<T, KS>())[rw] : 1.0f;
        pt[e] = pt_in[d];
        const int64_t t = obj_idx[d];
        tgt[e] = (int)(t < 0 ? 0 : (t >= N ? N - 1 : t));
    }
    int cnt[16];
    float bce[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        cnt[e] = 0;
        bce[e] = 0.f;
    }
    Frag<T, KS> f;
    if (g0 < g1) f.load(O, min(g0 * 32 + r, N - 1), c, h, vec);
    for (int g = g0; g < g1; ++g) {
        const int j = g * 32 + r;
        f.template convert<SG>();
        if (g + 1 < g1) f.load(O, min(j + 32, N - 1), c, h, vec);   // next group's rows in flight under the chain
        const f32x16 acc = f.chain(A0, A1);
        if (j < N) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = f.template prob<SG>(acc[e], srow[e]);
                cnt[e] += (p > pt[e]) + ((p == pt[e]) & (j < tgt[e]));
                if (BCE) bce[e] += clog(1.0f - p);
            }
        }
    }
    // rows: reduce over the 32 columns of each half wave (a fixed tree), lane 0 / 32 writes its 16 rows
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            cnt[e] += __shfl_xor(cnt[e], o);
            if (BCE) bce[e] += __shfl_xor(bce[e], o);
        }
    }
    if (r == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int d = mt * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
            if (d < B) {
                part_cnt[(int64_t)chunk * B + d] = cnt[e];
                if (BCE) part_bce[(int64_t)chunk * B + d] = bce[e];
            }
        }
    }
}

// entity ranges of the sweep: about 4096 waves in all (4 per SIMD), at least one 32-column group per range
int64_t n_chunks_of(int64_t batch, int64_t n_ent) {
    const int64_t n_mt = rtk_cdiv(batch, 32), G = rtk_cdiv(n_ent, 32);
    if (n_mt < 1) return 0;
    int64_t k = rtk_cdiv(4 * 4 * RTK_N_CU, n_mt);
    return k < G ? k : G;
}

struct RankLayout {
    size_t pt, cnt, bce, total;
};
RankLayout layout_of(int64_t batch, int64_t n_ent) {
    RankLayout L;
    const int64_t nch = n_chunks_of(batch, n_ent);
    L.pt = 256;                                               // [0, 256): the error word's header
    L.cnt = L.pt + rtk_align_up((size_t)batch * 4, 256);
    L.bce = L.cnt + rtk_align_up((size_t)(nch * batch) * 4, 256);
    L.total = L.bce + rtk_align_up((size_t)(nch * batch) * 4, 256);
    return L;
}

template <typename T, int KS, int SG>
int launch(const unsigned char *qp, int B, const T *O, int N, int c, const int64_t *obj_idx, const int64_t *pair_slot,
           const int64_t *pair_ptr, const int64_t *pair_obj, int32_t *ranks, double *bce_rows, unsigned char *ws,
           hipStream_t st) {
    const RankLayout L = layout_of(B, N);
    uint32_t *err = reinterpret_cast<uint32_t *>(ws);
    float *pt = reinterpret_cast<float *>(ws + L.pt);
    int32_t *pcnt = reinterpret_cast<int32_t *>(ws + L.cnt);
    float *pbce = reinterpret_cast<float *>(ws + L.bce);
    const int nch = (int)n_chunks_of(B, N);
    const bool vec = sizeof(T) == 4 || (c % 8 == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0);
    hipLaunchKernelGGL((pair_kernel<T, KS, SG, false>), dim3(B), dim3(64), 0, st, qp, B, O, N, c, obj_idx, pair_slot,
                       pair_ptr, pair_obj, pt, (const int32_t *)nullptr, (const float *)nullptr, 0, (int32_t *)nullptr,
                       (double *)nullptr, err, vec);
    const int64_t waves = rtk_cdiv(B, 32) * (int64_t)nch;
    const dim3 grid((unsigned)rtk_cdiv(waves, RK_WAVES));
    if (bce_rows)
        RTK_LAUNCH_SCORE((sweep_kernel<T, KS, SG, true>), grid, dim3(64 * RK_WAVES), 0, st, qp, B, O, N, c, obj_idx, pt,
                         nch, pcnt, pbce, vec);
    else
        RTK_LAUNCH_SCORE((sweep_kernel<T, KS, SG, false>), grid, dim3(64 * RK_WAVES), 0, st, qp, B, O, N, c, obj_idx, pt,
                         nch, pcnt, pbce, vec);
    hipLaunchKernelGGL((pair_kernel<T, KS, SG, true>), dim3(B), dim3(64), 0, st, qp, B, O, N, c, obj_idx, pair_slot,
                       pair_ptr, pair_obj, pt, pcnt, pbce, nch, ranks, bce_rows, err, vec);
    return RTK_OK;
}

template <typename T>
int score_rank(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_ent,
               const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
               unsigned flags, int32_t *ranks, double *bce_rows, void *workspace, size_t ws_bytes, void *stream) {
    constexpr bool F32 = sizeof(T) == 4;
    RTK_REQUIRE(q_packed && O && obj_idx && ranks && workspace, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", fn);
    RTK_REQUIRE(batch >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld must be >= 0", fn, (long long)batch);
    RTK_REQUIRE(n_ent >= 1, RTK_ERR_BAD_ARG, "%s: n_ent = %lld must be >= 1", fn, (long long)n_ent);
    RTK_REQUIRE(c >= 1, RTK_ERR_BAD_ARG, "%s: object rank c = %d must be >= 1", fn, c);
    RTK_REQUIRE(batch < (1ll << 31) - 32 && n_ent < (1ll << 31) - 64, RTK_ERR_UNSUPPORTED, "%s: dimension too large", fn);
    RTK_REQUIRE(flags & RTK_SCORE_SIGMOID, RTK_ERR_UNSUPPORTED,
                "%s: ranks are taken on probabilities: flags need RTK_SCORE_SIGMOID (raw logits are not ranked)", fn);
    RTK_REQUIRE((flags & ~(RTK_SCORE_SIGMOID | RTK_SCORE_SIGMOID_FAST)) == 0, RTK_ERR_BAD_ARG, "%s: unknown flags 0x%x",
                fn, flags);
    if (F32) {
        RTK_REQUIRE(c <= 16 * RK_MAX_KS_F32, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d (the ws kernel's range)", fn, c,
                    16 * RK_MAX_KS_F32);
        RTK_REQUIRE(c % 4 == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0, RTK_ERR_UNSUPPORTED,
                    "%s: fp32 needs c %% 4 == 0 and a 16-byte-aligned O (c = %d)", fn, c);
    } else {
        RTK_REQUIRE(c <= 16 * RK_MAX_KS_BF16, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d", fn, c, 16 * RK_MAX_KS_BF16);
    }
    const size_t need = layout_of(batch, n_ent).total;
    RTK_REQUIRE(ws_bytes >= need, RTK_ERR_BAD_ARG, "%s: workspace of %zu bytes given, %zu needed", fn, ws_bytes, need);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_BAD_ARG, "%s: workspace must be 256-byte aligned",
                fn);
    if (batch == 0) return RTK_OK;
    const int sg = (flags & RTK_SCORE_SIGMOID_FAST) ? 2 : 1;
    const int ks = (c + 15) / 16;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char *qp = (const unsigned char *)q_packed;
    unsigned char *ws = (unsigned char *)workspace;
    const int B = (int)batch, N = (int)n_ent;
    const int rc = rtk_dispatch_ksteps<F32 ? RK_MAX_KS_F32 : RK_MAX_KS_BF16>(ks, fn, [&](auto K) {
        if (sg == 2)
            return launch<T, K.value, 2>(qp, B, O, N, c, obj_idx, pair_slot, pair_ptr, pair_obj, ranks, bce_rows, ws, st);
        return launch<T, K.value, 1>(qp, B, O, N, c, obj_idx, pair_slot, pair_ptr, pair_obj, ranks, bce_rows, ws, st);
    });
    if (rc != RTK_OK) return rc;
    return rtk_check_launch(fn);
}

}  // namespace

extern "C" size_t rtk_score_rank_workspace_bytes(int dtype, int64_t batch, int64_t n_ent, int c) {
    (void)dtype;
    (void)c;
    if (batch < 0 || n_ent < 1) return 0;
    return layout_of(batch, n_ent).total;
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
