// The 1-vs-all softmax cross-entropy loss on STORED fp32 logits (the matrix form, beside rtk_bce.hip), targets as the
// CSR of known objects per (subject, relation) pair: with n_d the length of row d's list, t0 = eps / N and
// w_d = (1 - eps) [n_d > 0] + eps,
//   rtk_ce_rows_f32 : lse_d = log sum_j exp(z[d, j]) (row maximum subtracted) and
//                     rows[d] = w_d lse_d - t0 sum_j z[d, j] - (1 - eps) / n_d sum_{t in P_d} z[d, t]   (loss = sum / B)
//   rtk_ce_grad_f32 : Z <- (w_d exp(Z - lse_d) - y) * g * scale, in place, ready for the dO / dv GEMMs.
// One pass over the B x N logits each, plus a pass over the few positives.  Any c: the logits are whatever the caller
// stored (score_1vN(sigmoid=False)), with row pitch ld.
#include "rtk_common.h"

namespace {

constexpr float CE_L2E = 1.4426950408889634f;
constexpr float CE_NONE = -3.0e38f;

__device__ __forceinline__ float ce_exp(float a) { return __builtin_amdgcn_exp2f(a * CE_L2E); }

__device__ __forceinline__ void ce_list(int d, const int64_t *__restrict__ pair_slot, const int64_t *__restrict__ pair_ptr,
                                        int64_t &i0, int64_t &i1) {
    const int64_t s = pair_slot[d];
    i0 = s >= 0 ? pair_ptr[s] : 0;
    i1 = s >= 0 ? pair_ptr[s + 1] : 0;
    if (i1 < i0) i1 = i0;
}

// one workgroup per row: a thread keeps an online (maximum, sum of exp) over its columns, eight at a time (float within
// the eight, float64 across them); the threads' pairs are merged at the row maximum in a fixed order
__global__ __launch_bounds__(256) void ce_rows_kernel(const float *__restrict__ Z, int N, int64_t ld, double t0, double eps,
                                                      const int64_t *__restrict__ pair_slot,
                                                      const int64_t *__restrict__ pair_ptr,
                                                      const int64_t *__restrict__ pair_obj, double *__restrict__ rows,
                                                      float *__restrict__ lse_out) {
    __shared__ float s_max[4];
    __shared__ double s_sum[3][4];
    const int d = blockIdx.x, t = threadIdx.x;
    const float *row = Z + (int64_t)d * ld;
    constexpr int U = 8;                               // loads in flight per thread
    float M = CE_NONE;
    double S = 0.0, SZ = 0.0;
    for (int j = t; j < N; j += 256 * U) {
        float z[U];
        float m = M, zs = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = j + 256 * u < N;
            z[u] = in ? row[j + 256 * u] : CE_NONE;
            zs += in ? z[u] : 0.f;
            m = fmaxf(m, z[u]);
        }
        float ts = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) ts += z[u] > CE_NONE ? ce_exp(z[u] - m) : 0.f;
        S = S * (double)ce_exp(M - m) + (double)ts;
        M = m;
        SZ += (double)zs;
    }
    // the pair's known objects
    int64_t i0, i1;
    ce_list(d, pair_slot, pair_ptr, i0, i1);
    double PZ = 0.0;
    for (int64_t i = i0 + t; i < i1; i += 256) {
        const int64_t j = pair_obj[i];
        if (j >= 0 && j < N) PZ += (double)row[j];
    }
    float m = M;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((t & 63) == 0) s_max[t >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    double a = S > 0.0 ? S * exp((double)M - (double)m) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        SZ += __shfl_xor(SZ, o);
        PZ += __shfl_xor(PZ, o);
    }
    if ((t & 63) == 0) {
        s_sum[0][t >> 6] = a;
        s_sum[1][t >> 6] = SZ;
        s_sum[2][t >> 6] = PZ;
    }
    __syncthreads();
    if (t == 0) {
        const double s = ((s_sum[0][0] + s_sum[0][1]) + s_sum[0][2]) + s_sum[0][3];
        const double sz = ((s_sum[1][0] + s_sum[1][1]) + s_sum[1][2]) + s_sum[1][3];
        const double pz = ((s_sum[2][0] + s_sum[2][1]) + s_sum[2][2]) + s_sum[2][3];
        const double lse = (double)m + log(s);
        const int64_t n = i1 - i0;
        const double w = (n > 0 ? 1.0 - eps : 0.0) + eps;
        rows[d] = w * lse - t0 * sz - (n > 0 ? (1.0 - eps) / (double)n * pz : 0.0);
        lse_out[d] = (float)lse;
    }
}

// Pass 1, every element: z <- (w exp(z - lse) - t0) * g * scale (grid-stride over rows x column chunks)
template <bool VEC>
__global__ __launch_bounds__(256) void ce_grad_all_kernel(float *__restrict__ Z, int N, int64_t ld, float t0, float eps,
                                                          const int64_t *__restrict__ pair_slot,
                                                          const int64_t *__restrict__ pair_ptr,
                                                          const float *__restrict__ lse, const float *__restrict__ g,
                                                          float scale) {
    const float s = g[0] * scale;
    const int d = blockIdx.y;
    float *row = Z + (int64_t)d * ld;
    int64_t i0, i1;
    ce_list(d, pair_slot, pair_ptr, i0, i1);
    const float w = (i1 > i0 ? 1.0f - eps : 0.f) + eps, l = lse[d];
    if (VEC) {
        const int n4 = N >> 2;
        for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += gridDim.x * 256) {
            f32x4 x = reinterpret_cast<f32x4 *>(row)[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (w * ce_exp(x[e] - l) - t0) * s;
            reinterpret_cast<f32x4 *>(row)[q] = x;
        }
        for (int j = (n4 << 2) + blockIdx.x * 256 + threadIdx.x; j < N; j += gridDim.x * 256)
            row[j] = (w * ce_exp(row[j] - l) - t0) * s;
    } else {
        for (int j = blockIdx.x * 256 + threadIdx.x; j < N; j += gridDim.x * 256) row[j] = (w * ce_exp(row[j] - l) - t0) * s;
    }
}

// Pass 2, the positives: x <- x - (1 - eps) / n_d * g * scale (every object of a pair is listed once).  One workgroup per row.
__global__ __launch_bounds__(64) void ce_grad_pos_kernel(float *__restrict__ Z, int N, int64_t ld, float dt,
                                                         const int64_t *__restrict__ pair_slot,
                                                         const int64_t *__restrict__ pair_ptr,
                                                         const int64_t *__restrict__ pair_obj, const float *__restrict__ g,
                                                         float scale) {
    const int d = blockIdx.x;
    float *row = Z + (int64_t)d * ld;
    int64_t i0, i1;
    ce_list(d, pair_slot, pair_ptr, i0, i1);
    if (i1 <= i0) return;
    const float cf = dt / (float)(i1 - i0) * (g[0] * scale);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 64) {
        const int64_t j = pair_obj[i];
        if (j >= 0 && j < N) row[j] -= cf;
    }
}

int check(const char *fn, const float *Z, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
          const int64_t *pair_ptr, const int64_t *pair_obj, float eps) {
    RTK_REQUIRE(Z && pair_slot && pair_ptr && pair_obj, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(batch > 0 && n_ent > 0 && ld >= n_ent, RTK_ERR_BAD_ARG, "%s: bad sizes", fn);
    RTK_REQUIRE(eps >= 0.f && eps < 1.f, RTK_ERR_BAD_ARG, "%s: label smoothing %g outside [0, 1)", fn, (double)eps);
    RTK_REQUIRE(n_ent < (1ll << 31) - 256 * 8, RTK_ERR_UNSUPPORTED, "%s: dimension too large", fn);
    return RTK_OK;
}

}  // namespace

extern "C" int rtk_ce_rows_f32(const float *Z, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                               const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing, double *rows_out,
                               float *lse_out, void *stream) {
    int rc = check("rtk_ce_rows_f32", Z, batch, n_ent, ld, pair_slot, pair_ptr, pair_obj, label_smoothing);
    if (rc != RTK_OK) return rc;
    RTK_REQUIRE(rows_out && lse_out, RTK_ERR_BAD_ARG, "rtk_ce_rows_f32: null output");
    RTK_REQUIRE(batch < (1ll << 31), RTK_ERR_UNSUPPORTED, "rtk_ce_rows_f32: batch too large");
    hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, Z, (int)n_ent, ld,
                       (double)label_smoothing / (double)n_ent, (double)label_smoothing, pair_slot, pair_ptr, pair_obj,
                       rows_out, lse_out);
    return rtk_check_launch("rtk_ce_rows_f32");
}

extern "C" int rtk_ce_grad_f32(float *Z, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                               const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing, const float *lse,
                               const float *grad_loss, float scale, void *stream) {
    int rc = check("rtk_ce_grad_f32", Z, batch, n_ent, ld, pair_slot, pair_ptr, pair_obj, label_smoothing);
    if (rc != RTK_OK) return rc;
    RTK_REQUIRE(lse && grad_loss, RTK_ERR_BAD_ARG, "rtk_ce_grad_f32: null operand");
    RTK_REQUIRE(batch <= 65535, RTK_ERR_UNSUPPORTED, "rtk_ce_grad_f32: batch > 65535");
    const float t0 = label_smoothing / (float)n_ent, dt = 1.0f - label_smoothing;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(Z) & 15) == 0);
    const unsigned gx = (unsigned)(rtk_cdiv(n_ent, 1024 * 4) < 1 ? 1 : rtk_cdiv(n_ent, 1024 * 4));
    dim3 grid(gx < 64 ? gx : 64, (unsigned)batch);
    if (vec)
        hipLaunchKernelGGL((ce_grad_all_kernel<true>), grid, dim3(256), 0, st, Z, (int)n_ent, ld, t0, label_smoothing, pair_slot,
                           pair_ptr, lse, grad_loss, scale);
    else
        hipLaunchKernelGGL((ce_grad_all_kernel<false>), grid, dim3(256), 0, st, Z, (int)n_ent, ld, t0, label_smoothing,
                           pair_slot, pair_ptr, lse, grad_loss, scale);
    hipLaunchKernelGGL(ce_grad_pos_kernel, dim3((unsigned)batch), dim3(64), 0, st, Z, (int)n_ent, ld, dt, pair_slot, pair_ptr,
                       pair_obj, grad_loss, scale);
    return rtk_check_launch("rtk_ce_grad_f32");
}
