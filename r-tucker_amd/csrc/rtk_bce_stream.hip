// The 1-vs-all BCE training loss and its gradients without the (B, N) score matrix: the matrix-free form of
// rtk_score_packed_bce_f32 + rtk_bce_patch_pos_f32 (forward) and of the two B x N sized GEMMs of the backward.
// Everything is linear in the upstream gradient, so the sweeps work on the unscaled logit gradient of a negative,
//
//     x[d, j] = p[d, j] - eps / N        (0 where the fp32 p is exactly 1.0f or 0.0f),
//
// and the positives (the CSR entries, whose target is eps / N + (1 - eps)) are a sparse correction.  The skeletons of
// the three kernels are rtk_stream_kernel.h's (rows_sweep, GoSweep / go_kernel, pos_kernel), shared with the softmax
// cross-entropy loss (rtk_ce_stream.hip); this file holds the BCE link functions (BceRows, BceGo, BcePos) and the host:
//
//   rows_kernel   sweep 1.  The score tile is computed with the QUERY on the lane and the entities in the accumulator
//                 registers (entity fragments as the A operand, the packed query planes as B), so the 32 x 32 tile of x is
//                 the A operand of the next product, dv[d, :] += sum_j x[d, j] O[j, :], with no lane movement.  A
//                 workgroup of 4 waves holds 4 query tiles (fragments and the dv accumulators in registers) and sweeps
//                 a range of 32-row entity tiles; each tile is converted once per workgroup into LDS in two layouts
//                 (the chain's operand with the per-row scaling of Frag, and the k-permuted transposed operand of the
//                 dv product with one scale for all of O).  The BCE terms of the tile are summed per query.  The entity
//                 range is cut into `splits` parts; slabs and loss partials are added by finish_kernel in split order.
//   go_kernel     sweep 2, the entity-stationary sweep of rtk_score_rank_kernel.h: a wave converts its 32 entity rows
//                 once, sweeps the query tiles staged through LDS together with the packed tile of s v, and accumulates
//                 gO[j, :] += sum_d x[d, j] (s v[d, :]).  Here the entity is on the lane and the tile is the A operand
//                 of X^T V.  A wave owns its 32 rows of gO: one read-add-store on top of the positives' share.
//   pos_kernel    the positives: one workgroup per query re-scores the query's CSR entries with Frag (the sweeps' bits),
//                 gives the loss correction -(1 - eps) (ln p - ln(1 - p)), the positives' share of dv, and the flat
//                 (entity, query, dz) lists that the ordered scatter (rtk_scatter.h) turns into their share of gO.
//
// The block form (rtk_bce_stream_*_part_f32): O holds rows [col0, col0 + N) of an n_ent-row matrix.  The sweeps are
// row-local, so they only take the smoothing term eps / n_ent from the host; pos_kernel owns the CSR entries whose
// GLOBAL id falls into the block and works on local rows.  The whole-matrix entry points are the block launchers with
// col0 = 0, N = n_ent.
//
// Both tile products are three f16 MFMAs per k-step on hi/lo halves (x scaled by 2^14; O and s v by a power of two from
// their largest magnitude), accumulated in fp32.  No float atomics: every sum has a fixed order.
#include "rtk_bce_link.h"

namespace {

// sweep 1's link: the BCE terms of the tile summed per query, x = p - eps / N
template <int KS, int SG>
struct BceRows {
    float t0;
    double *__restrict__ part_loss;
    double lsum;
    __device__ __forceinline__ void begin(int, bool) { lsum = 0.0; }
    __device__ __forceinline__ void tile(const f32x16 &acc, float srow, const unsigned char *kc, int tile, int h, int N,
                                         float (&x)[16]) {
        float ls = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 kc4 = *reinterpret_cast<const f32x4 *>(kc + (8 * g + 4 * h) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                const bool valid = tile * 32 + 8 * g + 4 * h + q < N;
                const float p = Frag<float, KS>::template logistic<SG>(acc[e], srow, kc4[q]);
                x[e] = x_of(p, t0, valid);
                ls += valid ? t0 * rtk_clog(p) + (1.0f - t0) * rtk_clog(1.0f - p) : 0.f;
            }
        }
        lsum += (double)ls;
    }
    __device__ __forceinline__ void finish(int sp, int d, int h, int B) {
        lsum += __shfl_xor(lsum, 32);
        if (h == 0 && d < B) part_loss[(int64_t)sp * B + d] = lsum;
    }
};

// Sweep 1 (rows_sweep) with the BCE link.
template <int KS, int SG, bool DV>
__global__ __launch_bounds__(64 * BS_WAVES, 1) void rows_kernel(const unsigned char *__restrict__ qp, int B,
                                                                const float *__restrict__ O, int N, int c, float t0,
                                                                const float *__restrict__ o_bound, int n_splits,
                                                                double *__restrict__ part_loss,
                                                                float *__restrict__ slab) {
    BceRows<KS, SG> pol{t0, part_loss, 0.0};
    rows_sweep<KS, SG, DV>(pol, qp, B, O, N, c, o_bound, n_splits, slab);
}

// loss_rows[d] = -(the splits' partial sums, in split order) + the positives' correction;
// dv[d, :] = (the splits' slabs, in split order) * 2^-(14 + sh_O) + the positives' share.  One workgroup per query.
__global__ __launch_bounds__(256) void rows_finish_kernel(int B, int c, int cp, int n_splits,
                                                          const double *__restrict__ part_loss,
                                                          const double *__restrict__ rows_pos,
                                                          const float *__restrict__ slab, const float *__restrict__ dvpos,
                                                          const float *__restrict__ o_bound,
                                                          double *__restrict__ loss_rows, float *__restrict__ dv) {
    const int d = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        double s = 0.0;
        for (int k = 0; k < n_splits; ++k) s += part_loss[(int64_t)k * B + d];
        double pcor = 0.0;
#pragma unroll
        for (int u = 0; u < BS_POS_Y; ++u) pcor += rows_pos[(int64_t)d * BS_POS_Y + u];
        loss_rows[d] = -s + pcor;
    }
    finish_dv_row(d, t, B, c, cp, n_splits, slab, dvpos, o_bound, dv);
}

// ---- host side -------------------------------------------------------------------------------------------------

struct BceWs : StreamWs {
    size_t part_loss;
};
BceWs layout_of(int64_t batch, int c, int64_t max_pos) {
    BceWs L{stream_layout(batch, c, max_pos), 0};
    L.part_loss = L.take((size_t)splits_of(batch) * (size_t)batch * 8);
    return L;
}

// what rows and grad_o check alike (max_pos = 0 for rows)
int check_stream(const char *fn, const void *q_packed, int64_t batch, int c, const float *O, int64_t n_local, int64_t col0,
                 int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos, float eps,
                 unsigned flags, const void *out, const void *workspace, size_t ws_bytes) {
    const auto own = [&] { return check_pos_eps(fn, max_pos, eps); };
    return check_block(fn, q_packed && pair_slot && pair_ptr && pair_obj && out, batch, c, O, n_local, col0, n_ent, own,
                       (1ll << 31) - 256, flags, "the loss is", workspace, ws_bytes,
                       [&] { return layout_of(batch, c, max_pos).total; });
}

template <int KS, int SG>
int launch_rows(const unsigned char *qp, int B, int c, const float *O, int N, int col0, int n_ent, const int64_t *slot,
                const int64_t *ptr, const int64_t *obj, float eps, double *loss_rows, float *dv, unsigned char *ws,
                const BceWs &L, hipStream_t st, const char *fn) {
    const float t0 = eps / (float)n_ent, dt = 1.0f - eps;       // the smoothing term of the WHOLE entity count
    const int splits = splits_of(B), n_qg = (int)rtk_cdiv(rtk_cdiv(B, 32), BS_WAVES);
    float *bounds = reinterpret_cast<float *>(ws + L.bounds);
    double *part_loss = reinterpret_cast<double *>(ws + L.part_loss), *rows_pos = reinterpret_cast<double *>(ws + L.rows_pos);
    float *slab = reinterpret_cast<float *>(ws + L.slab), *dvpos = reinterpret_cast<float *>(ws + L.dvpos);
    if (dv) {
        const int rc = rtk_absmax_f32(O, N, c, c, bounds, (void *)st);
        if (rc != RTK_OK) return rc;
    }
    hipLaunchKernelGGL((pos_kernel<float, KS, SG, BcePos>), dim3((unsigned)B), dim3(64 * BS_WAVES), 0, st, qp, B, O, N, col0, c, dt, slot, ptr,
                       obj, rows_pos, dv ? dvpos : nullptr, (const int32_t *)nullptr, (int64_t)0, (int32_t *)nullptr,
                       (int32_t *)nullptr, (float *)nullptr);
    constexpr int bytes = RowsLds<KS>::TOTAL;
    static_assert(bytes <= 64 * 1024, "rows_kernel: one 32-row tile in two layouts fits the default LDS limit");
    const dim3 grid((unsigned)(n_qg * splits));
    if (dv)
        RTK_LAUNCH_SCORE((rows_kernel<KS, SG, true>), grid, dim3(64 * BS_WAVES), bytes, st, qp, B, O, N, c, t0, bounds, splits,
                         part_loss, slab);
    else
        RTK_LAUNCH_SCORE((rows_kernel<KS, SG, false>), grid, dim3(64 * BS_WAVES), bytes, st, qp, B, O, N, c, t0, bounds, splits,
                         part_loss, slab);
    hipLaunchKernelGGL(rows_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, B, c, 32 * nct_of(KS), splits, part_loss,
                       rows_pos, slab, dvpos, bounds, loss_rows, dv);
    return RTK_OK;
}

template <int KS, int SG>
int launch_grad_o(const unsigned char *qp, const float *v, int B, int c, const float *O, int N, int col0, int n_ent,
                  const int64_t *slot, const int64_t *ptr, const int64_t *obj, int64_t max_pos, float eps,
                  const float *scale, float *gO, unsigned char *ws, const BceWs &L, hipStream_t st, const char *fn) {
    return launch_go<KS, SG, BcePos>(qp, v, B, c, O, N, col0, slot, ptr, obj, max_pos, 1.0f - eps, scale,
                                     BceGo{eps / (float)n_ent}, (const unsigned char *)nullptr, gO, ws, L, st, fn);
}

// The two sweeps on rows [col0, col0 + n_local) of the (n_ent x c) matrix; the whole matrix is the block (0, n_ent).
int stream_rows(const char *fn, const void *q_packed, int64_t batch, int c, const float *O, int64_t n_local, int64_t col0,
                int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj, float eps,
                unsigned flags, double *loss_rows_out, float *dv_out, void *workspace, size_t ws_bytes, void *stream) {
    int rc = check_stream(fn, q_packed, batch, c, O, n_local, col0, n_ent, pair_slot, pair_ptr, pair_obj, 0, eps, flags,
                          loss_rows_out, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    const BceWs L = layout_of(batch, c, 0);
    return dispatch<float>(fn, c, flags, [&](auto K, auto SG) {
        return launch_rows<K.value, SG.value>((const unsigned char *)q_packed, (int)batch, c, O, (int)n_local, (int)col0,
                                              (int)n_ent, pair_slot, pair_ptr, pair_obj, eps, loss_rows_out, dv_out,
                                              (unsigned char *)workspace, L, (hipStream_t)stream, fn);
    });
}

int stream_grad_o(const char *fn, const void *q_packed, const float *v, int64_t batch, int c, const float *O, int64_t n_local,
                  int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                  int64_t max_pos, float eps, unsigned flags, const float *scale, float *gO_out, void *workspace,
                  size_t ws_bytes, void *stream) {
    RTK_REQUIRE(v && scale, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    int rc = check_stream(fn, q_packed, batch, c, O, n_local, col0, n_ent, pair_slot, pair_ptr, pair_obj, max_pos, eps, flags,
                          gO_out, workspace, ws_bytes);
    if (rc != RTK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0) return zero_go(fn, gO_out, n_local, c, st);
    const BceWs L = layout_of(batch, c, max_pos);
    return dispatch<float>(fn, c, flags, [&](auto K, auto SG) {
        return launch_grad_o<K.value, SG.value>((const unsigned char *)q_packed, v, (int)batch, c, O, (int)n_local, (int)col0,
                                                (int)n_ent, pair_slot, pair_ptr, pair_obj, max_pos, eps, scale, gO_out,
                                                (unsigned char *)workspace, L, st, fn);
    });
}

}  // namespace

extern "C" size_t rtk_bce_stream_workspace_bytes(int64_t batch, int64_t n_ent, int c, int64_t max_pos) {
    return stream_shape_ok(batch, n_ent, c, max_pos) ? layout_of(batch, c, max_pos).total : 0;
}

extern "C" size_t rtk_bce_stream_part_workspace_bytes(int64_t batch, int64_t n_local, int c, int64_t max_pos) {
    return rtk_bce_stream_workspace_bytes(batch, n_local, c, max_pos);
}

extern "C" int rtk_bce_stream_rows_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_ent,
                                       const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                       float label_smoothing, unsigned flags, double *loss_rows_out, float *dv_out,
                                       void *workspace, size_t ws_bytes, void *stream) {
    return stream_rows("rtk_bce_stream_rows_f32", q_packed, batch, c, O, n_ent, 0, n_ent, pair_slot, pair_ptr, pair_obj,
                       label_smoothing, flags, loss_rows_out, dv_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_bce_stream_rows_part_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                            int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                            const int64_t *pair_obj, float label_smoothing, unsigned flags,
                                            double *loss_rows_out, float *dv_out, void *workspace, size_t ws_bytes,
                                            void *stream) {
    return stream_rows("rtk_bce_stream_rows_part_f32", q_packed, batch, c, O_local, n_local, col0, n_ent, pair_slot, pair_ptr,
                       pair_obj, label_smoothing, flags, loss_rows_out, dv_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_bce_stream_grad_o_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O,
                                         int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                         const int64_t *pair_obj, int64_t max_pos, float label_smoothing, unsigned flags,
                                         const float *scale, float *gO_out, void *workspace, size_t ws_bytes, void *stream) {
    return stream_grad_o("rtk_bce_stream_grad_o_f32", q_packed, v, batch, c, O, n_ent, 0, n_ent, pair_slot, pair_ptr, pair_obj,
                         max_pos, label_smoothing, flags, scale, gO_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_bce_stream_grad_o_part_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O_local,
                                              int64_t n_local, int64_t col0, int64_t n_ent, const int64_t *pair_slot,
                                              const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos,
                                              float label_smoothing, unsigned flags, const float *scale, float *gO_local_out,
                                              void *workspace, size_t ws_bytes, void *stream) {
    return stream_grad_o("rtk_bce_stream_grad_o_part_f32", q_packed, v, batch, c, O_local, n_local, col0, n_ent, pair_slot,
                         pair_ptr, pair_obj, max_pos, label_smoothing, flags, scale, gO_local_out, workspace, ws_bytes, stream);
}
