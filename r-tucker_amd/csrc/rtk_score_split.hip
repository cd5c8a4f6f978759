// Stage 2 of the scoring path on the bf16/fp16-rate matrix cores:
//     out[d, j] = sigmoid( v[d,:] . O[j,:] )         (reference: asymmetric/R_TuckER.py:47-48)
//
// fp32 operands are evaluated as a split-precision product on v_mfma_f32_32x32x16_f16:
// x = hi + lo (two fp16 halves of a power-of-two-scaled row, ~22 significand bits) and
//     v.o  ~=  vh.oh + vh.ol + vl.oh           (fp32 accumulation inside the MFMA)
// -- 3 MFMAs at 16x the fp32-MFMA rate, i.e. 5.3x the throughput of an exact fp32 MFMA
// GEMM at about fp32 accuracy (the dropped vl.ol term is 2^-22 relative).  That moves
// this kernel from matrix-core-bound (fp32) to the HBM write of the B x N scores.
//
// Work decomposition ("entity-stationary"): a workgroup of 4 waves owns 128 entity
// rows of O; each wave converts ITS 32 rows once into register-resident B fragments
// (row max -> power-of-two scale -> hi/lo split; O is read from HBM exactly once and
// never written back), then the workgroup sweeps the query tiles: each 32-query tile
// of packed planes (rtk_pack.h) is copied linearly into LDS, every wave reads the same
// A fragments (conflict-free ds_read_b128) and issues 3*KS MFMAs into one 32x32
// accumulator, and the epilogue unscales, applies the logistic and stores
// 128-B-contiguous row segments (lane = entity) straight from the accumulator.
#include <string.h>

#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_select.h"

#include "rtk_score_split_kernel.h"
using rtk_split::score_split_kernel;
namespace {

// Minimum resident waves per SIMD of the instantiation: two 4-wave workgroups per CU up to c = 256; for
// 256 < c <= 512 (the doubled-rank tensors the Riemannian gradient scores) one, the hi/lo B
// fragments take up to 256 of a wave's 512 registers (the compiler places them in the accumulation half of the
// unified file)
constexpr int min_waves(int ks) { return ks <= 16 ? 2 : 1; }

template <int KS, int SG, int MINW>
int launch_one(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld,
                bool o_vec, unsigned grid, hipStream_t st) {
    constexpr size_t smem = 2 * (size_t)(RTK_PACK_HDR + 2 * KS * 1024);
    static std::atomic<unsigned long long> lds_ok{0};
    if (smem > 64 * 1024) {
        const int rc = rtk_ensure_dynamic_lds(reinterpret_cast<const void *>(&score_split_kernel<KS, SG, MINW, 0>), (int)smem,
                                              lds_ok, "score_split_kernel");
        if (rc != RTK_OK) return rc;
    }
    hipLaunchKernelGGL((score_split_kernel<KS, SG, MINW, 0>), dim3(grid), dim3(256), smem, st, qp, B, O, N, c,
                       out, ld, o_vec);
    return RTK_OK;
}

template <int KS, int MINW>
int launch_ks(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld,
               int sigmoid, bool o_vec, hipStream_t st) {
    // one block per resident slot (256 CUs x MINW workgroups); the kernel splits the
    // linearised (entity tile, query tile) space evenly over them
    const int64_t units = rtk_cdiv(N, 128) * rtk_cdiv(B, 32);
    const unsigned grid = (unsigned)(units < RTK_N_CU * MINW ? units : RTK_N_CU * MINW);
    if (sigmoid == 0) return launch_one<KS, 0, MINW>(qp, B, O, N, c, out, ld, o_vec, grid, st);
    if (sigmoid == 1) return launch_one<KS, 1, MINW>(qp, B, O, N, c, out, ld, o_vec, grid, st);
    return launch_one<KS, 2, MINW>(qp, B, O, N, c, out, ld, o_vec, grid, st);
}

// training forward: x = p - t0 and the negatives' BCE terms (score_split_kernel<..., LOSS = true>)
template <int KS, int MINW>
int launch_loss(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld, bool o_vec, float t0,
                double *partials, hipStream_t st) {
    constexpr size_t smem = 2 * (size_t)(RTK_PACK_HDR + 2 * KS * 1024);
    static std::atomic<unsigned long long> lds_ok{0};
    if (smem > 64 * 1024) {
        const int rc = rtk_ensure_dynamic_lds(reinterpret_cast<const void *>(&score_split_kernel<KS, 2, MINW, 0, true>), (int)smem,
                                              lds_ok, "score_split_kernel (loss)");
        if (rc != RTK_OK) return rc;
    }
    const int64_t units = rtk_cdiv(N, 128) * rtk_cdiv(B, 32);
    const unsigned grid = (unsigned)(units < RTK_N_CU * MINW ? units : RTK_N_CU * MINW);
    hipLaunchKernelGGL((score_split_kernel<KS, 2, MINW, 0, true>), dim3(grid), dim3(256), smem, st, qp, B, O, N, c, out, ld,
                       o_vec, t0, partials);
    return RTK_OK;
}

}  // namespace

extern "C" int rtk_score_packed_f32(const void *q_packed, int64_t batch, int c, const float *O,
                                    int64_t n_local, float *out, int64_t ld_out, unsigned flags,
                                    void *stream) {
    RTK_REQUIRE(q_packed && O && out, RTK_ERR_BAD_ARG, "rtk_score_packed_f32: null operand");
    RTK_REQUIRE(batch > 0 && n_local > 0 && c > 0, RTK_ERR_BAD_ARG, "rtk_score_packed_f32: sizes must be positive");
    RTK_REQUIRE(ld_out >= n_local, RTK_ERR_BAD_ARG, "rtk_score_packed_f32: ld_out < n_local");
    RTK_REQUIRE(ld_out < (1ll << 24), RTK_ERR_UNSUPPORTED, "rtk_score_packed_f32: ld_out >= 2^24 (32 rows must fit a 2 GiB buffer window)");
    RTK_REQUIRE(batch < (1ll << 31) && n_local < (1ll << 31) - 256, RTK_ERR_UNSUPPORTED, "rtk_score_packed_f32: dimension too large");
    RTK_REQUIRE(rtk_split_ksteps_supported(c), RTK_ERR_UNSUPPORTED, "rtk_score_packed_f32: c=%d > 512 not supported by the split-fp16 kernel (use rtk_score_f32)", c);
    hipStream_t st = (hipStream_t)stream;
    const int ks = (c + 15) / 16;
    const int sg = !(flags & RTK_SCORE_SIGMOID) ? 0 : ((flags & RTK_SCORE_SIGMOID_FAST) ? 2 : 1);
    const bool o_vec = (c % 4 == 0) && ((reinterpret_cast<uintptr_t>(O) & 15) == 0);
    const int B = (int)batch, N = (int)n_local;
    const unsigned char *qp = (const unsigned char *)q_packed;
    const RtkScorePlan plan = rtk_score_plan_f32(N, c, o_vec, flags);
    int rc;
    switch (plan.kernel) {
    case RTK_SCORE_KERNEL_CG:
        rc = sg == 0   ? rtk_score_cg_launch<0>(qp, B, O, N, c, out, ld_out, plan, st)
             : sg == 1 ? rtk_score_cg_launch<1>(qp, B, O, N, c, out, ld_out, plan, st)
                       : rtk_score_cg_launch<2>(qp, B, O, N, c, out, ld_out, plan, st);
        break;
    case RTK_SCORE_KERNEL_WS: rc = rtk_score_ws_launch(qp, B, O, N, c, out, ld_out, sg, st); break;
    default:
        rc = rtk_dispatch_ksteps<32>(ks, "rtk_score_packed_f32", [&](auto K) {
            return launch_ks<K.value, min_waves(K.value)>(qp, B, O, N, c, out, ld_out, sg, o_vec, st);
        });
    }
    if (rc != RTK_OK) return rc;
    return rtk_check_launch("rtk_score_packed_f32");
}

// Host-only queries of the plan above, for a 16-byte-aligned O (no device is touched).
static int query_plan(const char *what, int64_t n_local, int c, unsigned flags, RtkScorePlan *plan) {
    RTK_REQUIRE(n_local > 0 && n_local < (1ll << 31) - 256 && rtk_split_ksteps_supported(c), RTK_ERR_BAD_ARG,
                "%s: n_local=%lld c=%d outside the split-fp16 kernels' shapes", what, (long long)n_local, c);
    *plan = rtk_score_plan_f32(n_local, c, c % 4 == 0, flags);
    return RTK_OK;
}

extern "C" int rtk_score_kernel_f32(int64_t n_local, int c, unsigned flags) {
    RtkScorePlan plan;
    const int rc = query_plan("rtk_score_kernel_f32", n_local, c, flags, &plan);
    return rc != RTK_OK ? rc : (int)plan.kernel;
}

extern "C" int64_t rtk_score_fifth_group_columns_f32(int64_t n_local, int c, unsigned flags, unsigned char *mask) {
    RtkScorePlan plan;
    const int rc = query_plan("rtk_score_fifth_group_columns_f32", n_local, c, flags, &plan);
    if (rc != RTK_OK) return rc;
    if (mask) memset(mask, 0, (size_t)n_local);
    if (plan.kernel != RTK_SCORE_KERNEL_CG) return 0;
    // set u of U holds groups [G u / U, G (u + 1) / U) (rtk_score_cg_kernel.h, Geo::first_group); a set of five
    // computes its fifth group as four K-range chains
    const int64_t G = rtk_cdiv(n_local, 32), U = plan.U;
    int64_t cols = 0;
    for (int64_t u = 0; u < U; ++u) {
        const int64_t gb = G * u / U, ge = G * (u + 1) / U;
        if (ge - gb != RTK_CG_GROUPS_PER_SET) continue;
        const int64_t j0 = (gb + 4) * 32, j1 = (gb + 5) * 32 < n_local ? (gb + 5) * 32 : n_local;
        if (mask) memset(mask + j0, 1, (size_t)(j1 - j0));
        cols += j1 - j0;
    }
    return cols;
}

extern "C" int rtk_score_bce_partials(void) { return 512; }      // >= the largest grid of the loss kernel

extern "C" int rtk_score_packed_bce_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_local,
                                        float *x_out, int64_t ld_out, float label_smoothing, double *partials_out,
                                        void *stream) {
    RTK_REQUIRE(q_packed && O && x_out && partials_out, RTK_ERR_BAD_ARG, "rtk_score_packed_bce_f32: null operand");
    RTK_REQUIRE(batch > 0 && n_local > 0 && c > 0, RTK_ERR_BAD_ARG, "rtk_score_packed_bce_f32: sizes must be positive");
    RTK_REQUIRE(ld_out >= n_local, RTK_ERR_BAD_ARG, "rtk_score_packed_bce_f32: ld_out < n_local");
    RTK_REQUIRE(ld_out < (1ll << 24), RTK_ERR_UNSUPPORTED, "rtk_score_packed_bce_f32: ld_out >= 2^24");
    RTK_REQUIRE(batch < (1ll << 31) && n_local < (1ll << 31) - 256, RTK_ERR_UNSUPPORTED, "rtk_score_packed_bce_f32: dimension too large");
    RTK_REQUIRE(rtk_split_ksteps_supported(c), RTK_ERR_UNSUPPORTED, "rtk_score_packed_bce_f32: c=%d > 512 not supported", c);
    RTK_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, RTK_ERR_BAD_ARG, "rtk_score_packed_bce_f32: label smoothing %g outside [0, 1)", (double)label_smoothing);
    hipStream_t st = (hipStream_t)stream;
    const int zrc = rtk_zero_async("rtk_score_packed_bce_f32", partials_out, 512 * sizeof(double), st);
    if (zrc != RTK_OK) return zrc;
    const int ks = (c + 15) / 16;
    const bool o_vec = (c % 4 == 0) && ((reinterpret_cast<uintptr_t>(O) & 15) == 0);
    const int B = (int)batch, N = (int)n_local;
    const float t0 = label_smoothing / (float)n_local;
    const unsigned char *qp = (const unsigned char *)q_packed;
    const int rc = rtk_dispatch_ksteps<32>(ks, "rtk_score_packed_bce_f32", [&](auto K) {
        return launch_loss<K.value, min_waves(K.value)>(qp, B, O, N, c, x_out, ld_out, o_vec, t0, partials_out, st);
    });
    if (rc != RTK_OK) return rc;
    return rtk_check_launch("rtk_score_packed_bce_f32");
}
