// The matrix-free 1-vs-all BCE training loss on a block of bf16 entity rows, c <= 512: rtk_bce_stream.hip's two sweeps
// and positives with bf16 operands (O_local and the packed planes), without a (B, n_local) block and without an fp32
// copy of O_local.  The skeletons are rtk_stream_bf16_kernel.h's (rows_sweep_bf16, GoSweepBf16 / go_bf16_kernel) and
// rtk_stream_kernel.h's (pos_kernel, the images of s v, the flat lists, the ordered scatter); the links are
// rtk_bce_link.h's.  This file holds sweep 1's link and the host.
//
//     z = sum_k bf16(v)_k O_jk     summed as Frag<rtk_bf16, KS>::chain_with sums it: p has the bits of rtk_score_packed_bf16,
//     x = p - eps / n_ent          (0 where the fp32 p is exactly 1.0f or 0.0f; n_ent the GLOBAL entity count),
//     dv = X O,  gO = X^T (scale v) with the fp32 v of the call, not its bf16 rounding.
//
// The second tile product of both sweeps is cut along the output columns into chunks of at most 128 (blockIdx.y); each
// chunk computes the score tile again and only chunk 0 of sweep 1 forms the loss partials.  x is split into f16 hi/lo
// at 2^14; O enters as one fp16 plane (a bf16 value times the power of two of max |O| is exact in fp16 above the
// subnormals), scale v as f16 hi/lo (pack_v_kernel).  No float atomics: every sum has a fixed order.
#include "rtk_bce_link.h"
#include "rtk_stream_bf16_kernel.h"

namespace {

// sweep 1's link: the BCE terms of the tile summed per query (chunk 0 only), x = p - eps / n_ent
template <int KS, int SG>
struct BceRowsBf16 {
    float t0;
    double *__restrict__ part_loss;
    bool loss;                                                      // (workgroup-uniform: blockIdx.y == 0)
    double lsum;
    __device__ __forceinline__ void begin(int, bool) { lsum = 0.0; }
    __device__ __forceinline__ void tile(const f32x16 &acc, int tile, int h, int N, float (&x)[16]) {
        float p[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            p[e] = Frag<rtk_bf16, KS>::template prob<SG>(acc[e], 1.0f);
            x[e] = x_of(p[e], t0, tile * 32 + acc_row(e, h) < N);
        }
        if (loss) {
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                ls += tile * 32 + acc_row(e, h) < N ? t0 * rtk_clog(p[e]) + (1.0f - t0) * rtk_clog(1.0f - p[e]) : 0.f;
            lsum += (double)ls;
        }
    }
    __device__ __forceinline__ void finish(int sp, int d, int h, int B) {
        if (!loss) return;
        lsum += __shfl_xor(lsum, 32);
        if (h == 0 && d < B) part_loss[(int64_t)sp * B + d] = lsum;
    }
};

// Sweep 1 (rows_sweep_bf16) with the BCE link.
template <int KS, int SG, bool DV>
__global__ __launch_bounds__(64 * BS_WAVES, 1) void rows_bf16_kernel(const unsigned char *__restrict__ qp, int B,
                                                                     const rtk_bf16 *__restrict__ O, int N, int c, float t0,
                                                                     const float *__restrict__ o_bound, int n_splits,
                                                                     double *__restrict__ part_loss,
                                                                     float *__restrict__ slab) {
    BceRowsBf16<KS, SG> pol{t0, part_loss, blockIdx.y == 0, 0.0};
    rows_sweep_bf16<KS, SG, DV>(pol, qp, B, O, N, c, o_bound, n_splits, slab);
}

// rows_finish_kernel (rtk_bce_stream.hip) for up to 512 columns.  One workgroup per query.
__global__ __launch_bounds__(256) void rows_finish_bf16_kernel(int B, int c, int cp, int n_splits,
                                                               const double *__restrict__ part_loss,
                                                               const double *__restrict__ rows_pos,
                                                               const float *__restrict__ slab,
                                                               const float *__restrict__ dvpos,
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
    for (int col = t; col < c; col += 256) finish_dv_row(d, col, B, c, cp, n_splits, slab, dvpos, o_bound, dv);
}

// ---- host side -------------------------------------------------------------------------------------------------

struct BceBf16Ws : StreamWs {
    size_t part_loss;
};
BceBf16Ws layout_of(int64_t batch, int c, int64_t max_pos) {
    BceBf16Ws L{stream_layout(batch, c, max_pos, nctp_of((c + 15) / 16)), 0};
    L.part_loss = L.take((size_t)splits_of(batch) * (size_t)batch * 8);
    return L;
}

// what rows and grad_o check alike (max_pos = 0 for rows)
int check_stream(const char *fn, const void *q_packed, int64_t batch, int c, const rtk_bf16 *O, int64_t n_local, int64_t col0,
                 int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos,
                 float eps, unsigned flags, const void *out, const void *workspace, size_t ws_bytes) {
    const auto own = [&]() -> int {
        const int rc = check_pos_eps(fn, max_pos, eps);
        if (rc != RTK_OK) return rc;
        RTK_REQUIRE(vec_rows(O, c), RTK_ERR_UNSUPPORTED, "%s: bf16 needs c %% 8 == 0 and a 16-byte-aligned O (c = %d)", fn, c);
        return RTK_OK;
    };
    return check_block(fn, q_packed && pair_slot && pair_ptr && pair_obj && out, batch, c, O, n_local, col0, n_ent, own,
                       (1ll << 31) - 256, flags, "the loss is", workspace, ws_bytes,
                       [&] { return layout_of(batch, c, max_pos).total; });
}

template <int KS, int SG>
int launch_rows(const unsigned char *qp, int B, int c, const rtk_bf16 *O, int N, int col0, int n_ent, const int64_t *slot,
                const int64_t *ptr, const int64_t *obj, float eps, double *loss_rows, float *dv, unsigned char *ws,
                const BceBf16Ws &L, hipStream_t st, const char *fn) {
    const float t0 = eps / (float)n_ent, dt = 1.0f - eps;       // the smoothing term of the WHOLE entity count
    const int splits = splits_of(B), n_qg = (int)rtk_cdiv(rtk_cdiv(B, 32), BS_WAVES);
    float *bounds = reinterpret_cast<float *>(ws + L.bounds);
    double *part_loss = reinterpret_cast<double *>(ws + L.part_loss), *rows_pos = reinterpret_cast<double *>(ws + L.rows_pos);
    float *slab = reinterpret_cast<float *>(ws + L.slab), *dvpos = reinterpret_cast<float *>(ws + L.dvpos);
    if (dv) {
        const int rc = rtk_zero_async(fn, bounds, sizeof(float), st);
        if (rc != RTK_OK) return rc;
        const int64_t n = (int64_t)N * c;
        hipLaunchKernelGGL(absmax_bf16_kernel, dim3((unsigned)(rtk_cdiv(n, 8 * 256) < 1024 ? rtk_cdiv(n, 8 * 256) : 1024)),
                           dim3(256), 0, st, O, n, bounds);
    }
    hipLaunchKernelGGL((pos_kernel<rtk_bf16, KS, SG, BcePos>), dim3((unsigned)B), dim3(64 * BS_WAVES), 0, st, qp, B, O, N, col0,
                       c, dt, slot, ptr, obj, rows_pos, dv ? dvpos : nullptr, (const int32_t *)nullptr, (int64_t)0,
                       (int32_t *)nullptr, (int32_t *)nullptr, (float *)nullptr);
    constexpr int bytes = RowsLdsBf16<KS>::TOTAL;
    static_assert(bytes <= 64 * 1024, "rows_bf16_kernel: one 32-row tile and a chunk's image fit the default LDS limit");
    // without dv the chunks would only repeat the loss: chunk 0 alone
    const dim3 grid((unsigned)(n_qg * splits), dv ? (unsigned)nch_of(KS) : 1u);
    if (dv)
        RTK_LAUNCH_SCORE((rows_bf16_kernel<KS, SG, true>), grid, dim3(64 * BS_WAVES), bytes, st, qp, B, O, N, c, t0, bounds,
                         splits, part_loss, slab);
    else
        RTK_LAUNCH_SCORE((rows_bf16_kernel<KS, SG, false>), grid, dim3(64 * BS_WAVES), bytes, st, qp, B, O, N, c, t0, bounds,
                         splits, part_loss, slab);
    hipLaunchKernelGGL(rows_finish_bf16_kernel, dim3((unsigned)B), dim3(256), 0, st, B, c, 32 * nctp_of(KS), splits, part_loss,
                       rows_pos, slab, dvpos, bounds, loss_rows, dv);
    return RTK_OK;
}

template <int KS, int SG>
int launch_grad_o(const unsigned char *qp, const float *v, int B, int c, const rtk_bf16 *O, int N, int col0, int n_ent,
                  const int64_t *slot, const int64_t *ptr, const int64_t *obj, int64_t max_pos, float eps,
                  const float *scale, float *gO, unsigned char *ws, const BceBf16Ws &L, hipStream_t st, const char *fn) {
    const int rc = go_prologue<rtk_bf16, KS, SG, BcePos>(qp, v, B, c, nctp_of(KS), O, N, col0, slot, ptr, obj, max_pos,
                                                         1.0f - eps, scale, gO, ws, L, st, fn);
    if (rc != RTK_OK) return rc;
    // one workgroup per CU and chunk: whole entity tiles per slot, no query ranges
    const int n_slots = grid_of(B, N, RTK_N_CU).n_slots;
    return launch_lds<&go_bf16_kernel<KS, SG, BceGo>, GoLdsBf16<KS>::TOTAL>(
        dim3((unsigned)n_slots, (unsigned)nch_of(KS)), dim3(64 * BS_WAVES), st, fn, qp, (const unsigned char *)(ws + L.vp), B, O,
        N, c, BceGo{eps / (float)n_ent}, (const float *)(reinterpret_cast<const float *>(ws + L.bounds) + 1), gO);
}

bool shape_ok(int64_t batch, int64_t n_local, int c, int64_t max_pos) {
    return batch >= 0 && n_local >= 1 && c >= 1 && c <= 16 * BSB_MAX_KS && c % 8 == 0 && max_pos >= 0 &&
           max_pos < (1ll << 31) - 1;
}

}  // namespace

extern "C" size_t rtk_bce_stream_bf16_workspace_bytes(int64_t batch, int64_t n_local, int c, int64_t max_pos) {
    return shape_ok(batch, n_local, c, max_pos) ? layout_of(batch, c, max_pos).total : 0;
}

extern "C" int rtk_bce_stream_rows_part_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                             int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                             const int64_t *pair_obj, float label_smoothing, unsigned flags,
                                             double *loss_rows_out, float *dv_out, void *workspace, size_t ws_bytes,
                                             void *stream) {
    const char *fn = "rtk_bce_stream_rows_part_bf16";
    const rtk_bf16 *O = (const rtk_bf16 *)O_local;
    const int rc = check_stream(fn, q_packed, batch, c, O, n_local, col0, n_ent, pair_slot, pair_ptr, pair_obj, 0,
                                label_smoothing, flags, loss_rows_out, workspace, ws_bytes);
    if (rc != RTK_OK || batch == 0) return rc;
    const BceBf16Ws L = layout_of(batch, c, 0);
    return dispatch<rtk_bf16>(fn, c, flags, [&](auto K, auto SG) {
        return launch_rows<K.value, SG.value>((const unsigned char *)q_packed, (int)batch, c, O, (int)n_local, (int)col0,
                                              (int)n_ent, pair_slot, pair_ptr, pair_obj, label_smoothing, loss_rows_out,
                                              dv_out, (unsigned char *)workspace, L, (hipStream_t)stream, fn);
    });
}

extern "C" int rtk_bce_stream_grad_o_part_bf16(const void *q_packed, const float *v, int64_t batch, int c, const void *O_local,
                                               int64_t n_local, int64_t col0, int64_t n_ent, const int64_t *pair_slot,
                                               const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos,
                                               float label_smoothing, unsigned flags, const float *scale, float *gO_local_out,
                                               void *workspace, size_t ws_bytes, void *stream) {
    const char *fn = "rtk_bce_stream_grad_o_part_bf16";
    const rtk_bf16 *O = (const rtk_bf16 *)O_local;
    RTK_REQUIRE(v && scale, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    const int rc = check_stream(fn, q_packed, batch, c, O, n_local, col0, n_ent, pair_slot, pair_ptr, pair_obj, max_pos,
                                label_smoothing, flags, gO_local_out, workspace, ws_bytes);
    if (rc != RTK_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0) return zero_go(fn, gO_local_out, n_local, c, st);
    const BceBf16Ws L = layout_of(batch, c, max_pos);
    return dispatch<rtk_bf16>(fn, c, flags, [&](auto K, auto SG) {
        return launch_grad_o<K.value, SG.value>((const unsigned char *)q_packed, v, (int)batch, c, O, (int)n_local, (int)col0,
                                                (int)n_ent, pair_slot, pair_ptr, pair_obj, max_pos, label_smoothing, scale,
                                                gO_local_out, (unsigned char *)workspace, L, st, fn);
    });
}
