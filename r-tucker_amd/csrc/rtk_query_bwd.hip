// Backward of stage 1 (the query vectors), i.e. autograd of
//     v[d,:] = S[h_d,:] . ( G x_0 R[r_d,:] )            (reference: asymmetric/R_TuckER.py:43-46)
// given dv = d loss / d v  (B x c):
//     W[d,a,b]   = sum_c G[a,b,c] dv[d,c]                       GEMM  (B x c) . (ab x c)^T
//     gRb[d,a]   = sum_b W[d,a,b] S[h_d,b]
//     gSb[d,b]   = sum_a W[d,a,b] R[r_d,a]
//     gG[a,b,c]  = sum_d R[r_d,a] S[h_d,b] dv[d,c]              GEMM  X^T (ab x B) . dv (B x c),  X[d,(a,b)] = R[r_d,a] S[h_d,b]
//     gR[u,:]    = sum_{d: r_d = u} gRb[d,:]     gS[j,:] = sum_{d: h_d = j} gSb[d,:]
// The two GEMMs run on the exact-fp32 MFMA kernel (rtk_gemm_f32.hip).  The row scatter is
// DETERMINISTIC: the first query of every distinct id adds the rows of all queries with that id in
// increasing query order (no atomics, no index_add_), so two runs give bit-identical gradients.
#include "rtk_common.h"
#include "rtk_rows_scatter.h"   // clamp_id, SC_CB, scatter_rows_kernel: shared with rtk_query_bwd_stream.hip

int rtk_gemm_f32_ex(const void *A, int a_kmajor, int64_t lda, const int32_t *a_rows, const void *B,
                    int b_kmajor, int64_t ldb, float *C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                    unsigned flags, const uint32_t *m_dev, int in_bf16, hipStream_t st);

namespace {

// One workgroup per query: the two small contractions of W[d] and the Khatri-Rao row X[d].
__global__ __launch_bounds__(256) void bwd_rows_kernel(const float *__restrict__ W, int a, int b,
                                                       const float *__restrict__ R, int64_t n_rel,
                                                       const float *__restrict__ S, int64_t n_sub,
                                                       const int64_t *__restrict__ rel_idx,
                                                       const int64_t *__restrict__ sub_idx,
                                                       float *__restrict__ rows_R, float *__restrict__ rows_S,
                                                       float *__restrict__ X) {
    extern __shared__ float sm[];
    float *Rs = sm, *Ss = sm + a;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t d = blockIdx.x;
    const int64_t r = clamp_id(rel_idx[d], n_rel), h = clamp_id(sub_idx[d], n_sub);   // bad ids were flagged by the forward
    for (int i = t; i < a; i += 256) Rs[i] = R[r * a + i];
    for (int i = t; i < b; i += 256) Ss[i] = S[h * b + i];
    __syncthreads();
    const int64_t ab = (int64_t)a * b;
    const float *Wd = W + d * ab;
    if (rows_S) {
        for (int col = t; col < b; col += 256) {
            float acc = 0.f;
            for (int ai = 0; ai < a; ++ai) acc = fmaf(Wd[(int64_t)ai * b + col], Rs[ai], acc);
            rows_S[d * b + col] = acc;
        }
    }
    if (rows_R) {
        for (int ai = wave; ai < a; ai += 4) {
            float acc = 0.f;
            for (int col = lane; col < b; col += 64) acc = fmaf(Wd[(int64_t)ai * b + col], Ss[col], acc);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) rows_R[d * a + ai] = acc;
        }
    }
    if (X) {
        float *Xd = X + d * ab;
        for (int64_t i = t; i < ab; i += 256) Xd[i] = Rs[i / b] * Ss[i % b];
    }
}

struct BwdWs {
    float *W, *X, *rows_R, *rows_S;
    void *slabs;          // split-K slabs of the core-gradient GEMM
    size_t slab_bytes;
    int splits;
    size_t total;
};
// g_core = X^T dv is (a b) x c with K = batch: at the WN18RR rank that is 32 tiles of 128 x 128 for 256 CUs
// (63 us); K is cut until the tiles fill the chip (slabs added in chunk order: deterministic).
int gcore_splits(int64_t batch, int a, int b, int c) {
    const int64_t tiles = rtk_cdiv((int64_t)a * b, 128) * rtk_cdiv(c, 128);
    int64_t s = 256 / (tiles > 0 ? tiles : 1);
    if (s > batch / 64) s = batch / 64;
    return (int)(s < 1 ? 1 : (s > 16 ? 16 : s));
}
BwdWs carve_bwd(void *base, int64_t batch, int a, int b, int c) {
    BwdWs w;
    unsigned char *p = (unsigned char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char *q = p ? p + off : nullptr;
        off += rtk_align_up(bytes, 256);
        return (float *)q;
    };
    const size_t ab = (size_t)a * b;
    w.W = take((size_t)batch * ab * 4);
    w.X = take((size_t)batch * ab * 4);
    w.rows_R = take((size_t)batch * a * 4);
    w.rows_S = take((size_t)batch * b * 4);
    w.splits = gcore_splits(batch, a, b, c);
    w.slab_bytes = w.splits > 1 ? rtk_gemm_f32_splitk_workspace_bytes((int64_t)ab, c, w.splits) : 0;
    w.slabs = take(w.slab_bytes);
    w.total = off;
    return w;
}

}  // namespace

extern "C" size_t rtk_query_bwd_workspace_bytes(int64_t batch, int a, int b, int c) {
    if (batch <= 0 || a <= 0 || b <= 0 || c <= 0) return 0;
    return carve_bwd(nullptr, batch, a, b, c).total;
}

extern "C" int rtk_query_vectors_bwd_f32(const float *core, int a, int b, int c, const float *R, int64_t n_rel,
                                         const float *S, int64_t n_sub, const int64_t *rel_idx,
                                         const int64_t *sub_idx, int64_t batch, const float *dv, float *g_core,
                                         float *g_R, float *g_S, void *workspace, size_t workspace_bytes,
                                         void *stream) {
    const char *fn = "rtk_query_vectors_bwd_f32";
    RTK_REQUIRE(core && R && S && rel_idx && sub_idx && dv, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(a > 0 && b > 0 && c > 0 && n_rel > 0 && n_sub > 0 && batch > 0, RTK_ERR_BAD_ARG, "%s: sizes must be positive", fn);
    RTK_REQUIRE(batch < (1ll << 30), RTK_ERR_UNSUPPORTED, "%s: batch too large", fn);
    RTK_REQUIRE(n_rel < (1ll << 31) && n_sub < (1ll << 31), RTK_ERR_UNSUPPORTED, "%s: more than 2^31-1 rows", fn);
    RTK_REQUIRE(a <= 256 * SC_CB && b <= 256 * SC_CB, RTK_ERR_UNSUPPORTED, "%s: rank above %d not supported (a=%d b=%d)", fn, 256 * SC_CB, a, b);
    RTK_REQUIRE((size_t)(a + b) * 4 <= 64 * 1024, RTK_ERR_UNSUPPORTED, "%s: a + b too large for LDS", fn);
    const size_t need = rtk_query_bwd_workspace_bytes(batch, a, b, c);
    RTK_REQUIRE(workspace && workspace_bytes >= need, RTK_ERR_WORKSPACE, "%s: workspace of %zu bytes given, %zu needed", fn, workspace_bytes, need);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", fn);
    if (!g_core && !g_R && !g_S) return RTK_OK;
    hipStream_t st = (hipStream_t)stream;
    const BwdWs ws = carve_bwd(workspace, batch, a, b, c);
    const int64_t ab = (int64_t)a * b;
    int rc;
    if (g_R || g_S) {
        // W (B x ab) = dv (B x c, K-major) . core viewed as (ab x c, K-major)^T
        rc = rtk_gemm_f32_ex(dv, 1, c, nullptr, core, 1, c, ws.W, ab, batch, ab, c, 0, nullptr, 0, st);
        if (rc != RTK_OK) return rc;
    }
    hipLaunchKernelGGL(bwd_rows_kernel, dim3((unsigned)batch), dim3(256), (size_t)(a + b) * 4, st, ws.W, a, b, R, n_rel, S,
                       n_sub, rel_idx, sub_idx, g_R ? ws.rows_R : nullptr, g_S ? ws.rows_S : nullptr,
                       g_core ? ws.X : nullptr);
    if (g_core) {
        // gG (ab x c) = X^T . dv : A(m,k) = X[k*ab + m] (M-major), B(n,k) = dv[k*c + n] (M-major), K = B in query order
        if (ws.splits > 1)
            rc = rtk_gemm_f32_splitk(ws.X, 0, ab, dv, 0, c, g_core, c, ab, c, batch, ws.splits, ws.slabs, ws.slab_bytes, st);
        else
            rc = rtk_gemm_f32_ex(ws.X, 0, ab, nullptr, dv, 0, c, g_core, c, ab, c, batch, 0, nullptr, 0, st);
        if (rc != RTK_OK) return rc;
    }
    if (g_R && (rc = rtk_zero_async(fn, g_R, (size_t)n_rel * a * 4, st)) != RTK_OK) return rc;
    if (g_S && (rc = rtk_zero_async(fn, g_S, (size_t)n_sub * b * 4, st)) != RTK_OK) return rc;
    if (g_R || g_S)
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)(2 * batch)), dim3(256), 0, st, sub_idx, ws.rows_S, b, g_S, n_sub,
                           rel_idx, ws.rows_R, a, g_R, n_rel, (int)batch);
    return rtk_check_launch(fn);
}
