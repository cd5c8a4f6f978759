// Backward of stage 1 without the (B, a*b) intermediates: the second form of rtk_query_vectors_bwd_f32
// (rtk_query_bwd.hip), for shapes where W[d,i,j] = sum_k G[i,j,k] dv[d,k] and the Khatri-Rao operand do not fit.
//
//   gather_rows_kernel        Rg[d,:] = R[r_d,:], Sg[d,:] = S[h_d,:] as fp32 (ids clamped as bwd_rows_kernel does; a bf16
//                             row converts exactly).  B x (a + b) floats: all the later steps read.
//   g_core                    rtk_core_outer_f32(Rg, Sg, dv): the Khatri-Rao operand is formed while it is staged.
//   stream_rows_kernel        a workgroup owns 128 queries x 128 columns j of the core (one "b-tile") and walks i = 0 .. a-1.
//                             For every i it forms the 128 x 128 tile W[d, i, j] on v_mfma_f32_32x32x2_f32, exactly as
//                             rtk_gemm_f32 would (dv and G[i, b-tile, :] staged through LDS in k-tiles of 16, the next
//                             k-tile's loads in flight under the MFMAs), and uses it in registers:
//                               acc_S[d, j] = fmaf(W, Rg[d, i], acc_S)          held over the whole i loop -> rows_S
//                               part[bt, d, i] = sum over the tile's j of W * Sg[d, j]
//                             W never leaves the registers.  Wave w owns queries 32 w .. 32 w + 31 of the tile and all 128
//                             columns (four 32 x 32 MFMA tiles), so the sum over j stays inside a wave.
//   stream_finish_kernel      rows_R[d, i] = part[0, d, i] + part[1, d, i] + ... (b-tiles ascending).
//   scatter_rows_kernel       the ordered row scatter of rtk_query_bwd.hip (rtk_rows_scatter.h: one text, the same bits).
//
// THE ORDER OF THE SUMS
//   W[d,i,j]     one chain over k ascending from zero, fmaf per k (fp32 MFMA), the last k-tile zero-padded.
//   rows_S[d,j]  one chain fmaf(W[d,i,j], Rg[d,i], acc) over i ascending from zero: bwd_rows_kernel's chain, so g_S has
//                the values of rtk_query_vectors_bwd_f32 on every input.
//   rows_R[d,i]  per b-tile of 128 columns (j0 = 128 bt): lane r = 0 .. 31 forms
//                  p_r = W[j0+r] Sg[j0+r], then fmaf(W[j0+r+32], Sg[j0+r+32], p_r), then + 64, then + 96
//                (columns past b count as zeros), and the 32 lane sums are combined by a butterfly: p_r += p_(r xor 16),
//                then xor 8, 4, 2, 1.  The tiles' sums are added in ascending tile order, starting from tile 0's.
//                The bits depend on Sg[d], dv[d], the core and the tile width 128 alone -- not on the batch size nor on
//                the query's place in it (an MFMA output does not depend on its row, the butterfly is over columns).
//   g_core       rtk_core_outer_f32's: one chain over d ascending, no split-K.
// No float atomics; two runs give the same bits.
#include "rtk_common.h"
#include "rtk_rows_scatter.h"

namespace {

constexpr int QM = 128, QN = 128, QK = 16, QLD = 132;      // tile (queries x columns), k-tile, padded LDS row (floats)

template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T *__restrict__ R, int64_t n_rel, int a,
                                                          const T *__restrict__ S, int64_t n_sub, int b,
                                                          const int64_t *__restrict__ rel_idx,
                                                          const int64_t *__restrict__ sub_idx, float *__restrict__ Rg,
                                                          float *__restrict__ Sg) {
    const int t = threadIdx.x;
    const int64_t d = blockIdx.x;
    const int64_t r = clamp_id(rel_idx[d], n_rel), h = clamp_id(sub_idx[d], n_sub);   // bad ids were flagged by the forward
    for (int i = t; i < a; i += 256) Rg[d * a + i] = rtk_to_f32(R[r * a + i]);
    for (int i = t; i < b; i += 256) Sg[d * b + i] = rtk_to_f32(S[h * b + i]);
}

// 8 consecutive k of one row of a K-major operand, zero past K and for a row outside the operand
template <typename T>
__device__ __forceinline__ void load_row8(float (&s)[8], const T *__restrict__ row, bool row_in, int k, int K, bool vec) {
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = 0.f;
    if (!row_in || k >= K) return;
    const T *p = row + k;
    if (vec && k + 8 <= K) {
        const f32x4 x0 = rtk_load4(p), x1 = rtk_load4(p + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[q] = x0[q];
            s[4 + q] = x1[q];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (k + q < K) s[q] = rtk_to_f32(p[q]);
    }
}

// C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int acc_row_of(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

template <typename T>
__global__ __launch_bounds__(256) void stream_rows_kernel(const T *__restrict__ core, int a, int b, int c, bool g_vec,
                                                          const float *__restrict__ dv, bool dv_vec, int B,
                                                          const float *__restrict__ Rg, const float *__restrict__ Sg,
                                                          int n_bt, float *__restrict__ rows_S, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[QK * QLD];      // dv      [k][query]
    __shared__ __attribute__((aligned(16))) float Bs[QK * QLD];      // G[i]    [k][column]
    const int bt = (int)(blockIdx.x % (unsigned)n_bt), qt = (int)(blockIdx.x / (unsigned)n_bt);
    const int tile_m = qt * QM, tile_n = bt * QN;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int row0 = tile_m + 32 * wave;                             // the wave's first query

    // the tile of Sg the wave multiplies W with, in the accumulators' layout; zeros outside the operand
    float sreg[4][16];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int d = row0 + acc_row_of(e, h), j = tile_n + 32 * jb + r;
            sreg[jb][e] = (part && d < B && j < b) ? Sg[(int64_t)d * b + j] : 0.f;
        }
    f32x16 w[4], acc_s[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
        for (int e = 0; e < 16; ++e) w[jb][e] = acc_s[jb][e] = 0.f;

    // staging: thread t owns row t & 127 of both operands' tiles and k in [kh, kh + 8)
    const int srow = t & 127, kh = 8 * (t >> 7);
    const bool dq_in = tile_m + srow < B, gj_in = tile_n + srow < b;
    const float *dv_row = dv + (int64_t)(dq_in ? tile_m + srow : 0) * c;
    const int gj = gj_in ? tile_n + srow : 0;
    float sa[8], sb[8];
    auto load = [&](int i, int k0) {
        load_row8(sa, dv_row, dq_in, k0 + kh, c, dv_vec);
        load_row8(sb, core + ((int64_t)i * b + gj) * c, gj_in, k0 + kh, c, g_vec);
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            As[(kh + q) * QLD + srow] = sa[q];
            Bs[(kh + q) * QLD + srow] = sb[q];
        }
    };

    float rv[16];
    load(0, 0);
    stash();
    __syncthreads();
    for (int i = 0; i < a; ++i) {
        for (int k0 = 0; k0 < c; k0 += QK) {
            const bool last = k0 + QK >= c;                          // the last k-tile of this i
            const bool more = !last || i + 1 < a;
            if (more) load(last ? i + 1 : i, last ? 0 : k0 + QK);
            if (last) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int d = row0 + acc_row_of(e, h);
                    rv[e] = d < B ? Rg[(int64_t)d * a + i] : 0.f;
                }
            }
#pragma unroll
            for (int ks = 0; ks < QK / 2; ++ks) {
                const int kk = 2 * ks + h;
                const float x = As[kk * QLD + 32 * wave + r];
#pragma unroll
                for (int jb = 0; jb < 4; ++jb)
                    w[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, Bs[kk * QLD + 32 * jb + r], w[jb], 0, 0, 0);
            }
            if (last) {
                if (rows_S) {
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc_s[jb][e] = fmaf(w[jb][e], rv[e], acc_s[jb][e]);
                }
                if (part) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        float p = __fmul_rn(w[0][e], sreg[0][e]);
#pragma unroll
                        for (int jb = 1; jb < 4; ++jb) p = fmaf(w[jb][e], sreg[jb][e], p);
#pragma unroll
                        for (int o = 16; o > 0; o >>= 1) p = __fadd_rn(p, __shfl_xor(p, o));
                        const int d = row0 + acc_row_of(e, h);
                        if (r == 0 && d < B) part[((int64_t)bt * B + d) * a + i] = p;
                    }
                }
#pragma unroll
                for (int jb = 0; jb < 4; ++jb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) w[jb][e] = 0.f;
            }
            __syncthreads();
            if (more) {
                stash();
                __syncthreads();
            }
        }
    }
    if (rows_S) {
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            const int j = tile_n + 32 * jb + r;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int d = row0 + acc_row_of(e, h);
                if (d < B && j < b) rows_S[(int64_t)d * b + j] = acc_s[jb][e];
            }
        }
    }
}

// rows_R[x] = part[0][x] + part[1][x] + ... over the b-tiles, ascending; x over the batch * a elements
__global__ __launch_bounds__(256) void stream_finish_kernel(const float *__restrict__ part, int64_t n, int n_bt,
                                                            float *__restrict__ rows_R) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += stride) {
        float s = part[x];
        for (int bt = 1; bt < n_bt; ++bt) s = __fadd_rn(s, part[(int64_t)bt * n + x]);
        rows_R[x] = s;
    }
}

struct StreamWs {
    float *Rg, *Sg, *rows_R, *rows_S, *part;
    int n_bt;
    size_t total;
};
StreamWs carve_stream(void *base, int64_t batch, int a, int b) {
    StreamWs w;
    unsigned char *p = (unsigned char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char *q = p ? p + off : nullptr;
        off += rtk_align_up(bytes, 256);
        return (float *)q;
    };
    w.n_bt = (int)rtk_cdiv(b, QN);
    w.Rg = take((size_t)batch * a * 4);
    w.Sg = take((size_t)batch * b * 4);
    w.rows_R = take((size_t)batch * a * 4);
    w.rows_S = take((size_t)batch * b * 4);
    w.part = take((size_t)w.n_bt * batch * a * 4);
    w.total = off;
    return w;
}

template <typename T>
int bwd_stream(const char *fn, const T *core, int a, int b, int c, const T *R, int64_t n_rel, const T *S, int64_t n_sub,
               const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch, const float *dv, float *g_core, float *g_R,
               float *g_S, void *workspace, size_t workspace_bytes, void *stream) {
    RTK_REQUIRE(core && R && S && rel_idx && sub_idx && dv, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(a > 0 && b > 0 && c > 0 && n_rel > 0 && n_sub > 0 && batch > 0, RTK_ERR_BAD_ARG, "%s: sizes must be positive", fn);
    RTK_REQUIRE(batch < (1ll << 30), RTK_ERR_UNSUPPORTED, "%s: batch too large", fn);
    RTK_REQUIRE(n_rel < (1ll << 31) && n_sub < (1ll << 31), RTK_ERR_UNSUPPORTED, "%s: more than 2^31-1 rows", fn);
    RTK_REQUIRE(a <= 256 * SC_CB && b <= 256 * SC_CB && c <= 256 * SC_CB, RTK_ERR_UNSUPPORTED,
                "%s: rank above %d not supported (a=%d b=%d c=%d)", fn, 256 * SC_CB, a, b, c);
    const size_t need = rtk_query_bwd_stream_workspace_bytes(batch, a, b, c);
    RTK_REQUIRE(workspace && workspace_bytes >= need, RTK_ERR_WORKSPACE, "%s: workspace of %zu bytes given, %zu needed", fn,
                workspace ? workspace_bytes : (size_t)0, need);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", fn);
    if (!g_core && !g_R && !g_S) return RTK_OK;
    hipStream_t st = (hipStream_t)stream;
    const StreamWs ws = carve_stream(workspace, batch, a, b);
    int rc;
    hipLaunchKernelGGL((gather_rows_kernel<T>), dim3((unsigned)batch), dim3(256), 0, st, R, n_rel, a, S, n_sub, b, rel_idx,
                       sub_idx, ws.Rg, ws.Sg);
    if (g_core) {
        rc = rtk_core_outer_f32(ws.Rg, a, a, ws.Sg, b, b, dv, c, c, batch, g_core, stream);
        if (rc != RTK_OK) return rc;
    }
    if (g_R || g_S) {
        constexpr uintptr_t VA = rtk_vec4_align<T>();
        const bool g_vec = (reinterpret_cast<uintptr_t>(core) & (VA - 1)) == 0 && c % 4 == 0;
        const bool dv_vec = (reinterpret_cast<uintptr_t>(dv) & 15) == 0 && c % 4 == 0;
        const int64_t blocks = rtk_cdiv(batch, QM) * ws.n_bt;
        hipLaunchKernelGGL((stream_rows_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, core, a, b, c, g_vec, dv, dv_vec,
                           (int)batch, (const float *)ws.Rg, (const float *)ws.Sg, ws.n_bt, g_S ? ws.rows_S : nullptr,
                           g_R ? ws.part : nullptr);
        if (g_R) {
            const int64_t n = batch * a, fb = rtk_cdiv(n, 256);
            hipLaunchKernelGGL(stream_finish_kernel, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(256), 0, st,
                               (const float *)ws.part, n, ws.n_bt, ws.rows_R);
        }
        if (g_R && (rc = rtk_zero_async(fn, g_R, (size_t)n_rel * a * 4, st)) != RTK_OK) return rc;
        if (g_S && (rc = rtk_zero_async(fn, g_S, (size_t)n_sub * b * 4, st)) != RTK_OK) return rc;
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)(2 * batch)), dim3(256), 0, st, sub_idx, ws.rows_S, b, g_S, n_sub,
                           rel_idx, ws.rows_R, a, g_R, n_rel, (int)batch);
    }
    return rtk_check_launch(fn);
}

}  // namespace

extern "C" size_t rtk_query_bwd_stream_workspace_bytes(int64_t batch, int a, int b, int c) {
    if (batch <= 0 || a <= 0 || b <= 0 || c <= 0) return 0;
    return carve_stream(nullptr, batch, a, b).total;
}

extern "C" int rtk_query_vectors_bwd_stream_f32(const float *core, int a, int b, int c, const float *R, int64_t n_rel,
                                                const float *S, int64_t n_sub, const int64_t *rel_idx,
                                                const int64_t *sub_idx, int64_t batch, const float *dv, float *g_core,
                                                float *g_R, float *g_S, void *workspace, size_t workspace_bytes,
                                                void *stream) {
    return bwd_stream<float>("rtk_query_vectors_bwd_stream_f32", core, a, b, c, R, n_rel, S, n_sub, rel_idx, sub_idx, batch, dv,
                             g_core, g_R, g_S, workspace, workspace_bytes, stream);
}

extern "C" int rtk_query_vectors_bwd_stream_bf16(const void *core, int a, int b, int c, const void *R, int64_t n_rel,
                                                 const void *S, int64_t n_sub, const int64_t *rel_idx,
                                                 const int64_t *sub_idx, int64_t batch, const float *dv, float *g_core,
                                                 float *g_R, float *g_S, void *workspace, size_t workspace_bytes,
                                                 void *stream) {
    return bwd_stream<rtk_bf16>("rtk_query_vectors_bwd_stream_bf16", (const rtk_bf16 *)core, a, b, c, (const rtk_bf16 *)R, n_rel,
                                (const rtk_bf16 *)S, n_sub, rel_idx, sub_idx, batch, dv, g_core, g_R, g_S, workspace,
                                workspace_bytes, stream);
}
