// The 1-vs-all softmax cross-entropy training loss and its gradients without the (B, N) logit matrix: the sweeps of
// rtk_bce_stream.hip (rtk_stream_kernel.h) with another link function.  With P_d the CSR list of query d, n_d its
// length, t0 = eps / N and w_d = (1 - eps) [n_d > 0] + eps (the mass of the row's targets),
//
//     loss_rows[d] = w_d lse_d - t0 sum_j z[d, j] - (1 - eps) / n_d sum_{t in P_d} z[d, t],
//     x[d, j]      = w_d exp(z[d, j] - lse_d) - t0      (every valid column: there is no saturation rule),
//
// and the positives are the sparse correction -(1 - eps) / n_d per CSR entry.  z is Frag<float, KS>'s accumulated value
// times the row and column factors, acc * (srow * 2^-sh): the logit of the score kernels, without the logistic.
//
//   ce_fwd_kernel    the forward, sweep 1 without the second tile product: each lane keeps an online (maximum, sum of
//                    exp) and the sum of z of its query over its 16 entities per tile; partials per split.
//   ce_finish_kernel merges the splits' partials in split order in float64 (ce_merge_splits), adds the positives' term
//                    (pos_kernel with the CE link) and gives loss_rows and lse.
//   ce_dv_kernel     backward sweep 1 with the second tile product: dv[d, :] = sum_j x[d, j] O[j, :].
//   go_kernel        backward sweep 2 with the CE link: the tile's 32 values of lse and w travel with the query tile.
//
// The block form (rtk_ce_stream_*_part_f32): O holds rows [col0, col0 + N) of an n_ent-row matrix.  The loss is NOT a
// sum over entities -- the row's log-sum-exp couples the blocks -- so the forward stops before the logarithm and gives
// the block's (maximum, sum of exp at that maximum, linear part); the caller merges the blocks and hands the GLOBAL lse
// to the backward, which is the whole-matrix backward on the block's rows (t0 = eps / n_ent, n_d the stored list length,
// pos_kernel owning the CSR entries whose global id falls into the block).  The whole-matrix gradient entry point is
// the block launcher with col0 = 0, N = n_ent.
//
//   ce_part_finish_kernel  the same merge of the splits (ce_merge_splits), without the logarithm and without w.
//
// Every sum has a fixed order; no float atomics; nothing grows with B x N.
#include "rtk_stream_kernel.h"

namespace {

constexpr int CE_SG = 1;                        // plain column factors 2^-sh (no logistic is taken)
constexpr float CE_L2E = 1.4426950408889634f;
constexpr float CE_NONE = -3.0e38f;             // the running maximum before the first valid column

__device__ __forceinline__ float ce_exp(float a) { return __builtin_amdgcn_exp2f(a * CE_L2E); }

// the mass of query d's targets and the weight of one of its positives
__device__ __forceinline__ int64_t ce_list_len(int d, const int64_t *__restrict__ pair_slot,
                                               const int64_t *__restrict__ pair_ptr) {
    const int64_t s = pair_slot[d];
    const int64_t n = s >= 0 ? pair_ptr[s + 1] - pair_ptr[s] : 0;
    return n > 0 ? n : 0;
}

// the forward's link: online log-sum-exp and the sum of z per query
template <int KS>
struct CeFwdRows {
    float *__restrict__ part_max;
    double *__restrict__ part_sum, *__restrict__ part_z;
    float M;
    double S, SZ;
    __device__ __forceinline__ void begin(int, bool) {
        M = CE_NONE;
        S = SZ = 0.0;
    }
    __device__ __forceinline__ void tile(const f32x16 &acc, float srow, const unsigned char *kc, int tile, int h, int N,
                                         float (&)[16]) {
        float z[16];
        float m = M, zs = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kc4 = *reinterpret_cast<const f32x4 *>(kc + (8 * g + 4 * h) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                const bool valid = tile * 32 + 8 * g + 4 * h + q < N;
                z[e] = valid ? acc[e] * (srow * kc4[q]) : CE_NONE;      // a column past N: -inf for the lse, 0 for the sum
                zs += valid ? z[e] : 0.f;
                m = fmaxf(m, z[e]);
            }
        }
        float ts = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) ts += z[e] > CE_NONE ? ce_exp(z[e] - m) : 0.f;
        S = S * (double)ce_exp(M - m) + (double)ts;
        M = m;
        SZ += (double)zs;
    }
    __device__ __forceinline__ void finish(int sp, int d, int h, int B) {
        const float Mo = __shfl_xor(M, 32);
        const double So = __shfl_xor(S, 32), SZo = __shfl_xor(SZ, 32);
        if (h == 0 && d < B) {                                     // the lane pair's halves, h = 0 first
            const float m = fmaxf(M, Mo);
            const int64_t at = (int64_t)sp * B + d;
            part_max[at] = m;
            part_sum[at] = S * (double)ce_exp(M - m) + So * (double)ce_exp(Mo - m);
            part_z[at] = SZ + SZo;
        }
    }
};

// backward sweep 1's link: x from the query's lse and w (one query per lane)
template <int KS>
struct CeDvRows {
    const float *__restrict__ lw;               // per query tile: 32 lse, 32 w
    float t0;
    float lse, w;
    __device__ __forceinline__ void begin(int d, bool on) {
        lse = on ? lw[(d >> 5) * 64 + (d & 31)] : 0.f;
        w = on ? lw[(d >> 5) * 64 + 32 + (d & 31)] : 0.f;
    }
    __device__ __forceinline__ void tile(const f32x16 &acc, float srow, const unsigned char *kc, int tile, int h, int N,
                                         float (&x)[16]) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kc4 = *reinterpret_cast<const f32x4 *>(kc + (8 * g + 4 * h) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                const bool valid = tile * 32 + 8 * g + 4 * h + q < N;
                x[e] = valid ? w * ce_exp(acc[e] * (srow * kc4[q]) - lse) - t0 : 0.f;
            }
        }
    }
    __device__ __forceinline__ void finish(int, int, int, int) {}
};

template <int KS>
__global__ __launch_bounds__(64 * BS_WAVES, 1) void ce_fwd_kernel(const unsigned char *__restrict__ qp, int B,
                                                                  const float *__restrict__ O, int N, int c, int n_splits,
                                                                  float *__restrict__ part_max,
                                                                  double *__restrict__ part_sum,
                                                                  double *__restrict__ part_z) {
    CeFwdRows<KS> pol{part_max, part_sum, part_z, CE_NONE, 0.0, 0.0};
    rows_sweep<KS, CE_SG, false>(pol, qp, B, O, N, c, (const float *)nullptr, n_splits, (float *)nullptr);
}

template <int KS>
__global__ __launch_bounds__(64 * BS_WAVES, 1) void ce_dv_kernel(const unsigned char *__restrict__ qp, int B,
                                                                 const float *__restrict__ O, int N, int c, float t0,
                                                                 const float *__restrict__ lw,
                                                                 const float *__restrict__ o_bound, int n_splits,
                                                                 float *__restrict__ slab) {
    CeDvRows<KS> pol{lw, t0, 0.f, 0.f};
    rows_sweep<KS, CE_SG, true>(pol, qp, B, O, N, c, o_bound, n_splits, slab);
}

// The splits' partials of query d in split order, in float64: the maximum m, s = sum_k S_k exp(M_k - m) (a split
// without a tile has S_k = 0), sz = sum_k SZ_k, and the positives' term pcor.
__device__ __forceinline__ void ce_merge_splits(int d, int B, int n_splits, const float *__restrict__ part_max,
                                                const double *__restrict__ part_sum, const double *__restrict__ part_z,
                                                const double *__restrict__ rows_pos, float &m, double &s, double &sz,
                                                double &pcor) {
    m = CE_NONE;
    for (int k = 0; k < n_splits; ++k) m = fmaxf(m, part_max[(int64_t)k * B + d]);
    s = sz = 0.0;
    for (int k = 0; k < n_splits; ++k) {
        const int64_t at = (int64_t)k * B + d;
        const double sk = part_sum[at];
        if (sk > 0.0) s += sk * exp((double)part_max[at] - (double)m);
        sz += part_z[at];
    }
    pcor = 0.0;
#pragma unroll
    for (int u = 0; u < BS_POS_Y; ++u) pcor += rows_pos[(int64_t)d * BS_POS_Y + u];
}

// lse_d = m + ln s, then loss_rows[d] = w_d lse_d - t0 sz + the positives' term.  One thread per query.
__global__ __launch_bounds__(256) void ce_finish_kernel(int B, int n_splits, double t0, double eps,
                                                        const float *__restrict__ part_max,
                                                        const double *__restrict__ part_sum,
                                                        const double *__restrict__ part_z,
                                                        const double *__restrict__ rows_pos,
                                                        const int64_t *__restrict__ pair_slot,
                                                        const int64_t *__restrict__ pair_ptr,
                                                        double *__restrict__ loss_rows, float *__restrict__ lse_out) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= B) return;
    float m;
    double s, sz, pcor;
    ce_merge_splits(d, B, n_splits, part_max, part_sum, part_z, rows_pos, m, s, sz, pcor);
    const double lse = (double)m + log(s);
    const double w = (ce_list_len(d, pair_slot, pair_ptr) > 0 ? 1.0 - eps : 0.0) + eps;
    loss_rows[d] = w * lse - t0 * sz + pcor;
    lse_out[d] = (float)lse;
}

// The block form of ce_finish_kernel, stopped before the logarithm (the block does not know the other blocks):
// max_out[d] = m, sumexp_out[d] = s, lin_out[d] = -t0 sz + the positives' term of the block's entries.
__global__ __launch_bounds__(256) void ce_part_finish_kernel(int B, int n_splits, double t0,
                                                             const float *__restrict__ part_max,
                                                             const double *__restrict__ part_sum,
                                                             const double *__restrict__ part_z,
                                                             const double *__restrict__ rows_pos,
                                                             float *__restrict__ max_out, double *__restrict__ sumexp_out,
                                                             double *__restrict__ lin_out) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= B) return;
    float m;
    double s, sz, pcor;
    ce_merge_splits(d, B, n_splits, part_max, part_sum, part_z, rows_pos, m, s, sz, pcor);
    max_out[d] = m;
    sumexp_out[d] = s;
    lin_out[d] = -t0 * sz + pcor;
}

// lw of query tile mt: lse of its 32 queries, then their w; queries past B carry zeros
__global__ __launch_bounds__(256) void ce_lw_kernel(int B, int n_pad, float eps, const float *__restrict__ lse,
                                                    const int64_t *__restrict__ pair_slot,
                                                    const int64_t *__restrict__ pair_ptr, float *__restrict__ lw) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= n_pad) return;
    const bool in = d < B;
    lw[(d >> 5) * 64 + (d & 31)] = in ? lse[d] : 0.f;
    lw[(d >> 5) * 64 + 32 + (d & 31)] = in ? (ce_list_len(d, pair_slot, pair_ptr) > 0 ? 1.0f - eps : 0.f) + eps : 0.f;
}

// dv[d, :] = the splits' slabs + the positives' share.  One workgroup per query.
__global__ __launch_bounds__(256) void ce_dv_finish_kernel(int B, int c, int cp, int n_splits, const float *__restrict__ slab,
                                                           const float *__restrict__ dvpos,
                                                           const float *__restrict__ o_bound, float *__restrict__ dv) {
    finish_dv_row(blockIdx.x, threadIdx.x, B, c, cp, n_splits, slab, dvpos, o_bound, dv);
}

// the positives' link: every entry of a list of n carries (1 - eps) / n of the target mass; the loss is linear in z
struct CePos {
    static __device__ __forceinline__ float coef(float dt, int64_t n) { return n > 0 ? dt / (float)n : 0.f; }
    template <int SG, int KS>
    static __device__ __forceinline__ void term(const Frag<float, KS> &f, float acc, float srow, float cf, float &lacc,
                                                float &dz) {
        lacc += cf * (acc * (srow * f.kcol));
        dz = -cf;
    }
};

// sweep 2's link: the tile's 32 values of lse and of w travel behind the image of s v
struct CeGo {
    static constexpr int QB = 256;
    float t0;
    f32x4 l4, w4;
    __device__ __forceinline__ void rows4(const unsigned char *q4, int rw) {
        l4 = *reinterpret_cast<const f32x4 *>(q4 + rw * 4);
        w4 = *reinterpret_cast<const f32x4 *>(q4 + 128 + rw * 4);
    }
    template <int SG, int KS>
    __device__ __forceinline__ float x(const Frag<float, KS> &f, float acc, float srow, int q, bool valid) const {
        return valid ? w4[q] * ce_exp(acc * (srow * f.kcol) - l4[q]) - t0 : 0.f;
    }
};

// ---- host side -------------------------------------------------------------------------------------------------

struct CeWs : StreamWs {
    size_t part_max, part_sum, part_z, lw;
};
CeWs layout_of(int64_t batch, int c, int64_t max_pos) {
    CeWs L{stream_layout(batch, c, max_pos), 0, 0, 0, 0};
    const size_t SB = (size_t)splits_of(batch) * (size_t)batch;
    L.part_max = L.take(SB * 4);
    L.part_sum = L.take(SB * 8);
    L.part_z = L.take(SB * 8);
    L.lw = L.take((size_t)rtk_cdiv(batch, 32) * 256);
    return L;
}

int check_ce(const char *fn, bool operands, int64_t batch, int c, const float *O, int64_t n_local, int64_t col0, int64_t n_ent,
             int64_t max_pos, float eps, const void *workspace, size_t ws_bytes) {
    const auto own = [&] { return check_pos_eps(fn, max_pos, eps); };
    // (the entries take logits and have no flags: what = nullptr)
    return check_block(fn, operands, batch, c, O, n_local, col0, n_ent, own, (1ll << 31) - 256, 0u, (const char *)nullptr,
                       workspace, ws_bytes, [&] { return layout_of(batch, c, max_pos).total; });
}

// The forward on rows [col0, col0 + N) of the (n_ent x c) matrix.  The whole matrix (col0 = 0, N = n_ent) ends in
// ce_finish_kernel (loss_rows, lse); a block (part_max_out given) in ce_part_finish_kernel (maximum, sum of exp, linear part).
template <int KS>
int launch_fwd(const unsigned char *qp, int B, int c, const float *O, int N, int col0, int n_ent, const int64_t *slot,
               const int64_t *ptr, const int64_t *obj, float eps, double *loss_rows, float *lse, float *part_max_out,
               double *part_sumexp_out, double *part_lin_out, unsigned char *ws, const CeWs &L, hipStream_t st) {
    const int splits = splits_of(B), n_qg = (int)rtk_cdiv(rtk_cdiv(B, 32), BS_WAVES);
    float *part_max = reinterpret_cast<float *>(ws + L.part_max);
    double *part_sum = reinterpret_cast<double *>(ws + L.part_sum), *part_z = reinterpret_cast<double *>(ws + L.part_z);
    double *rows_pos = reinterpret_cast<double *>(ws + L.rows_pos);
    hipLaunchKernelGGL((pos_kernel<float, KS, CE_SG, CePos>), dim3((unsigned)B), dim3(64 * BS_WAVES), 0, st, qp, B, O, N, col0, c,
                       1.0f - eps, slot, ptr, obj, rows_pos, (float *)nullptr, (const int32_t *)nullptr, (int64_t)0,
                       (int32_t *)nullptr, (int32_t *)nullptr, (float *)nullptr);
    constexpr int bytes = RowsLds<KS>::TOTAL;
    static_assert(bytes <= 64 * 1024, "ce_fwd_kernel: one 32-row tile in two layouts fits the default LDS limit");
    RTK_LAUNCH_SCORE((ce_fwd_kernel<KS>), dim3((unsigned)(n_qg * splits)), dim3(64 * BS_WAVES), bytes, st, qp, B, O, N, c,
                     splits, part_max, part_sum, part_z);
    const double t0 = (double)eps / (double)n_ent;               // the smoothing term of the WHOLE entity count
    if (part_max_out)
        hipLaunchKernelGGL(ce_part_finish_kernel, dim3((unsigned)rtk_cdiv(B, 256)), dim3(256), 0, st, B, splits, t0,
                           (const float *)part_max, (const double *)part_sum, (const double *)part_z,
                           (const double *)rows_pos, part_max_out, part_sumexp_out, part_lin_out);
    else
        hipLaunchKernelGGL(ce_finish_kernel, dim3((unsigned)rtk_cdiv(B, 256)), dim3(256), 0, st, B, splits, t0, (double)eps,
                           (const float *)part_max, (const double *)part_sum, (const double *)part_z,
                           (const double *)rows_pos, slot, ptr, loss_rows, lse);
    return RTK_OK;
}

template <int KS>
int launch_grad(const unsigned char *qp, const float *v, int B, int c, const float *O, int N, int col0, int n_ent,
                const int64_t *slot, const int64_t *ptr, const int64_t *obj, int64_t max_pos, float eps, const float *lse,
                const float *scale, float *dv, float *gO, unsigned char *ws, const CeWs &L, hipStream_t st, const char *fn) {
    const float t0 = eps / (float)n_ent, dt = 1.0f - eps;        // the smoothing term of the WHOLE entity count
    constexpr int NCT = nct_of(KS);
    const int n_mt = (int)rtk_cdiv(B, 32), splits = splits_of(B), n_qg = (int)rtk_cdiv(n_mt, BS_WAVES);
    float *bounds = reinterpret_cast<float *>(ws + L.bounds);
    float *slab = reinterpret_cast<float *>(ws + L.slab), *dvpos = reinterpret_cast<float *>(ws + L.dvpos);
    float *lw = reinterpret_cast<float *>(ws + L.lw);
    hipLaunchKernelGGL(ce_lw_kernel, dim3((unsigned)rtk_cdiv(32 * n_mt, 256)), dim3(256), 0, st, B, 32 * n_mt, eps, lse, slot,
                       ptr, lw);
    if (dv) {                                                     // sweep 1 with the second tile product
        int rc = rtk_absmax_f32(O, N, c, c, bounds, (void *)st);
        if (rc != RTK_OK) return rc;
        hipLaunchKernelGGL((pos_kernel<float, KS, CE_SG, CePos>), dim3((unsigned)B), dim3(64 * BS_WAVES), 0, st, qp, B, O, N, col0, c, dt,
                           slot, ptr, obj, (double *)nullptr, dvpos, (const int32_t *)nullptr, (int64_t)0, (int32_t *)nullptr,
                           (int32_t *)nullptr, (float *)nullptr);
        constexpr int bytes = RowsLds<KS>::TOTAL;
        RTK_LAUNCH_SCORE((ce_dv_kernel<KS>), dim3((unsigned)(n_qg * splits)), dim3(64 * BS_WAVES), bytes, st, qp, B, O, N, c, t0,
                         (const float *)lw, (const float *)bounds, splits, slab);
        hipLaunchKernelGGL(ce_dv_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, B, c, 32 * NCT, splits,
                           (const float *)slab, (const float *)dvpos, (const float *)bounds, dv);
    }
    if (!gO) return RTK_OK;
    return launch_go<KS, CE_SG, CePos>(qp, v, B, c, O, N, col0, slot, ptr, obj, max_pos, dt, scale, CeGo{t0},
                                       (const unsigned char *)lw, gO, ws, L, st, fn);
}

template <typename F>
int dispatch_ce(const char *fn, int c, F f) {
    const int rc = rtk_dispatch_ksteps<SW_MAX_KS_F32>((c + 15) / 16, fn, f);
    return rc != RTK_OK ? rc : rtk_check_launch(fn);
}

// The gradients on rows [col0, col0 + n_local) of the (n_ent x c) matrix, from the GLOBAL lse; the whole matrix is the
// block (0, n_ent).
int stream_grad(const char *fn, const void *q_packed, const float *v, int64_t batch, int c, const float *O, int64_t n_local,
                int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                int64_t max_pos, float eps, const float *lse, const float *scale, float *dv_out, float *gO_out,
                void *workspace, size_t ws_bytes, void *stream) {
    RTK_REQUIRE(!gO_out || (v && scale), RTK_ERR_BAD_ARG, "%s: null operand", fn);
    int rc = check_ce(fn, q_packed && pair_slot && pair_ptr && pair_obj && lse && (dv_out || gO_out), batch, c, O, n_local, col0,
                      n_ent, max_pos, eps, workspace, ws_bytes);
    if (rc != RTK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0) return zero_go(fn, gO_out, n_local, c, st);
    const CeWs L = layout_of(batch, c, max_pos);
    return dispatch_ce(fn, c, [&](auto K) {
        return launch_grad<K.value>((const unsigned char *)q_packed, v, (int)batch, c, O, (int)n_local, (int)col0, (int)n_ent,
                                    pair_slot, pair_ptr, pair_obj, max_pos, eps, lse, scale, dv_out, gO_out,
                                    (unsigned char *)workspace, L, st, fn);
    });
}

}  // namespace

extern "C" size_t rtk_ce_stream_workspace_bytes(int64_t batch, int64_t n_ent, int c, int64_t max_pos) {
    return stream_shape_ok(batch, n_ent, c, max_pos) ? layout_of(batch, c, max_pos).total : 0;
}

extern "C" size_t rtk_ce_stream_part_workspace_bytes(int64_t batch, int64_t n_local, int c, int64_t max_pos) {
    return rtk_ce_stream_workspace_bytes(batch, n_local, c, max_pos);
}

extern "C" int rtk_ce_stream_rows_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_ent,
                                      const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                      float label_smoothing, double *loss_rows_out, float *lse_out, void *workspace,
                                      size_t ws_bytes, void *stream) {
    const char *fn = "rtk_ce_stream_rows_f32";
    int rc = check_ce(fn, q_packed && pair_slot && pair_ptr && pair_obj && loss_rows_out && lse_out, batch, c, O, n_ent, 0, n_ent,
                      0, label_smoothing, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    const CeWs L = layout_of(batch, c, 0);
    return dispatch_ce(fn, c, [&](auto K) {
        return launch_fwd<K.value>((const unsigned char *)q_packed, (int)batch, c, O, (int)n_ent, 0, (int)n_ent, pair_slot,
                                   pair_ptr, pair_obj, label_smoothing, loss_rows_out, lse_out, (float *)nullptr,
                                   (double *)nullptr, (double *)nullptr, (unsigned char *)workspace, L, (hipStream_t)stream);
    });
}

extern "C" int rtk_ce_stream_rows_part_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                           int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                           const int64_t *pair_obj, float label_smoothing, float *max_out,
                                           double *sumexp_out, double *lin_out, void *workspace, size_t ws_bytes,
                                           void *stream) {
    const char *fn = "rtk_ce_stream_rows_part_f32";
    int rc = check_ce(fn, q_packed && pair_slot && pair_ptr && pair_obj && max_out && sumexp_out && lin_out, batch, c, O_local,
                      n_local, col0, n_ent, 0, label_smoothing, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    const CeWs L = layout_of(batch, c, 0);
    return dispatch_ce(fn, c, [&](auto K) {
        return launch_fwd<K.value>((const unsigned char *)q_packed, (int)batch, c, O_local, (int)n_local, (int)col0, (int)n_ent,
                                   pair_slot, pair_ptr, pair_obj, label_smoothing, (double *)nullptr, (float *)nullptr, max_out,
                                   sumexp_out, lin_out, (unsigned char *)workspace, L, (hipStream_t)stream);
    });
}

extern "C" int rtk_ce_stream_grad_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O,
                                      int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                      const int64_t *pair_obj, int64_t max_pos, float label_smoothing, const float *lse,
                                      const float *scale, float *dv_out, float *gO_out, void *workspace, size_t ws_bytes,
                                      void *stream) {
    return stream_grad("rtk_ce_stream_grad_f32", q_packed, v, batch, c, O, n_ent, 0, n_ent, pair_slot, pair_ptr, pair_obj,
                       max_pos, label_smoothing, lse, scale, dv_out, gO_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_ce_stream_grad_part_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O_local,
                                           int64_t n_local, int64_t col0, int64_t n_ent, const int64_t *pair_slot,
                                           const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos,
                                           float label_smoothing, const float *lse, const float *scale, float *dv_out,
                                           float *gO_local_out, void *workspace, size_t ws_bytes, void *stream) {
    return stream_grad("rtk_ce_stream_grad_part_f32", q_packed, v, batch, c, O_local, n_local, col0, n_ent, pair_slot, pair_ptr,
                       pair_obj, max_pos, label_smoothing, lse, scale, dv_out, gO_local_out, workspace, ws_bytes, stream);
}
