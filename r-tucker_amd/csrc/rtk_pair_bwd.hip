// Relation prediction, backward: the gradients of the (h, ?, t) scores without a (B, a*b) buffer.
//
//   du = dZ . R and gR = dZ^T . u are ordinary GEMMs (rtk_gemm_f32).  What is new here:
//
//   rtk_pair_rows_f32    rows[d, j] = sum_i w[d, i] * sum_k core[i, j, k] X[x_idx[d], k]
//                        rS is this call on (core, O, t, du); rO is this call on the core with its last two axes
//                        transposed and (S, h, du).  It is the forward's sweep (rtk_pair.hip) with i and j exchanged.
//   rtk_core_outer_f32   gG[i, j, k] = sum_d (x[d, i] * y[d, j]) * z[d, k]: the exact fp32 MFMA GEMM whose left operand,
//                        the Khatri-Rao product of x and y, is formed while it is staged and never written to memory.
//   rtk_scatter_rows_f32 out[e, :] = sum_{d: idx[d] = e} rows[d, :]: a front end of the ordered scatter (rtk_scatter.h).
//
// rtk_pair_rows_f32, three launches on the caller's stream:
//
//   rows_gather_kernel   one workgroup per row of the query tiles: checks and clamps x_idx[d] (error word: 4), writes the
//                        packed planes of X[x_idx[d]] -- the layout and the bits rtk_pack_query_vectors gives for these
//                        rows -- and w[d, :] as fp32, zero-padded to a_pad columns.  Rows past the batch are zeros.
//   rows_kernel          the entity-stationary sweep (rtk_score_rank_kernel.h) with the core's rows as the "entities".
//                        Rows are indexed j * a_pad + i, a_pad = 32 ceil(a / 32), and read core row min(i, a - 1) * b + j:
//                        the 32 rows of a wave (one "chunk") belong to ONE j, the padding rows i >= a contribute 0.  A
//                        lane holds one row (i, j) and 16 queries: acc * (row factor * column factor) is
//                        sum_k core[i, j, k] X[x_d, k], times w[d, i] (read from the gathered rows), summed over the 32
//                        lanes by reduce16 and stored as the chunk's partial sum, part[mt][chunk][32 queries].  Nothing
//                        else is written: B * b * a_pad / 32 floats.
//   rows_finish_kernel   rows[d, j] = the a_pad / 32 partials of (d, j) added in ascending chunk order.
//
// The bits of rows[d, :] depend only on X[x_idx[d]], w[d, :] and the core.  An MFMA output element does not depend on
// its place in the tile, the planes' row factor is per query, reduce16 combines the 32 lanes of a chunk in one fixed
// tree whatever the element, every (query, chunk) partial has exactly one writer whatever the grid (qsplit only deals
// query tiles to workgroups), and rows_finish_kernel adds a query's partials in one order.  No atomics on data.
//
// rtk_core_outer_f32: ONE accumulation chain per output element, over d ascending from zero in k-tiles of 16 (the last
// one zero-padded), by v_mfma_f32_32x32x2_f32; no split-K.  So the bits do not depend on the tile shape or the grid and
// are those of rtk_gemm_f32 on the materialised left operand.
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_scatter.h"
#include "rtk_score_rank_kernel.h"

namespace {

__device__ __forceinline__ int64_t clamp_id(int64_t x, int64_t n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

// the largest of the workgroup's (256 threads) values, in every thread
__device__ __forceinline__ float block_max(float mx, float *red, int t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void rows_gather_kernel(const float *__restrict__ X, int64_t n_x,
                                                          const int64_t *__restrict__ x_idx, const float *__restrict__ w,
                                                          int64_t ld_w, int B, int a, int a_pad, int c, int ksteps,
                                                          unsigned char *__restrict__ planes, float *__restrict__ wg,
                                                          uint32_t *__restrict__ err) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const int64_t d = blockIdx.x;
    const bool live = d < B;                                          // workgroup-uniform
    int64_t xx = 0;
    if (live) {
        const int64_t x_raw = x_idx[d];
        xx = clamp_id(x_raw, n_x);
        if (t == 0 && xx != x_raw) atomicOr(err, 4u);
    }
    const float *wrow = w + (live ? d : 0) * ld_w;
    for (int i = t; i < a_pad; i += 256) wg[d * a_pad + i] = (live && i < a) ? wrow[i] : 0.f;
    const float *xrow = X + xx * c;
    const int cl = live ? c : 0;                                      // a row past the batch: zeros
    float mx = 0.f;
    for (int k = t; k < cl; k += 256) mx = fmaxf(mx, fabsf(xrow[k]));
    rtk_pack_store_row_f32(planes, d, ksteps, xrow, cl, block_max(mx, red, t), t, 256);
}

// What rows_kernel does with the sweep: nothing travels with a query tile; the 32 x 32 accumulators become a chunk's
// partial sums.
template <int KS>
struct RowsSweep {
    static constexpr int EXTRA = 0;
    int a, b, a_pad, na, n_chunks;                 // na = a_pad / 32 chunks per j, n_chunks = b * na
    const float *__restrict__ wg;                  // (32 n_mt, a_pad): w[d, :], zero-padded
    float *__restrict__ part;                      // (n_mt, n_chunks, 32)

    __device__ __forceinline__ void load_extra(SweepLane, int) const {}
    __device__ __forceinline__ void store_extra(SweepLane, int) const {}
    __device__ __forceinline__ void begin_tile() const {}
    __device__ __forceinline__ void end_tile(SweepLane, int) const {}
    __device__ __forceinline__ void publish(SweepLane, int, int, int, int, int, bool) const {}
    // row j * a_pad + i of the sweep reads row min(i, a - 1) * b + j of the core
    __device__ __forceinline__ int64_t row_of(int jl) const {
        const int j = jl / a_pad, i = jl - j * a_pad;
        return (int64_t)min(i, a - 1) * b + j;
    }
    __device__ __forceinline__ void score(SweepLane ln, const Frag<float, KS> &f, const f32x16 &acc,
                                          const unsigned char *buf, int, int jl, bool, int mt) const {
        const int r = ln.r, h = ln.h;
        const int chunk = __builtin_amdgcn_readfirstlane(jl >> 5);    // the wave's 32 rows: one j, i = 32 ic + r
        if (chunk >= n_chunks) return;                                // (wave-uniform) past the last row: the rows come in 32s
        const int i = (chunk % na) * 32 + r;
        const bool live = i < a;
        const float *wq = wg + (int64_t)mt * 32 * a_pad + i;
        float v[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rw = acc_row(4 * g, h);
            const f32x4 sr4 = *reinterpret_cast<const f32x4 *>(buf + rw * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                const float s = wq[(int64_t)(rw + q) * a_pad];
                const float x = acc[e] * (sr4[q] * f.kcol);
                v[e] = live ? x * s : 0.f;
            }
        }
        const float sum = reduce16(v, r, RedSum());
        if (!(r & 1)) part[((int64_t)mt * n_chunks + chunk) * 32 + red_row(r, h)] = sum;
    }
};

template <int KS>
__global__ __launch_bounds__(64 * SW_WAVES, 2) void rows_kernel(const unsigned char *__restrict__ planes, int B,
                                                                const float *__restrict__ core, int n_rows, int c, int a,
                                                                int b, int a_pad, const float *__restrict__ wg,
                                                                float *__restrict__ part, int n_slots, int qsplit) {
    RowsSweep<KS> pol{a, b, a_pad, a_pad >> 5, n_rows >> 5, wg, part};
    sweep<float, KS, 1>(pol, planes, B, core, n_rows, c, true, n_slots, qsplit);
}

// rows[d, j] = sum of the na partials of (d, j), ascending.  Workgroup (mt, y): the 32 queries of tile mt, j = 8 y .. 8 y + 7.
__global__ __launch_bounds__(256) void rows_finish_kernel(const float *__restrict__ part, int B, int b, int na,
                                                          float *__restrict__ rows, int64_t ld_rows) {
    const int t = threadIdx.x, rw = t & 31, j = (int)blockIdx.y * 8 + (t >> 5);
    const int mt = blockIdx.x, d = mt * 32 + rw;
    if (j >= b || d >= B) return;
    const float *p = part + (((int64_t)mt * b + j) * na) * 32 + rw;
    float s = p[0];
    for (int ic = 1; ic < na; ++ic) s += p[(int64_t)ic * 32];
    rows[d * ld_rows + j] = s;
}

// workspace: the error word's header, the planes of X[x_idx], the gathered w rows, the chunk partials
struct RowsLayout {
    int a_pad, na;
    int64_t n_mt, n_rows;
    size_t planes, wg, part, total;
};
RowsLayout rows_layout(int64_t batch, int a, int b, int c) {
    RowsLayout L;
    L.na = (a + 31) / 32;
    L.a_pad = 32 * L.na;
    L.n_mt = rtk_cdiv(batch, 32);
    L.n_rows = (int64_t)b * L.a_pad;
    L.planes = 256;
    L.wg = L.planes + rtk_align_up((size_t)L.n_mt * (size_t)rtk_pack_tile_bytes((c + 15) / 16, 2), 256);
    L.part = L.wg + rtk_align_up((size_t)L.n_mt * 32 * L.a_pad * 4, 256);
    L.total = L.part + rtk_align_up((size_t)L.n_mt * (size_t)b * L.na * 32 * 4, 256);
    return L;
}

// the shapes the sweep covers; fn == nullptr: only asked (no message)
int rows_check_shape(const char *fn, int64_t batch, int a, int b, int c, const void *core) {
    const bool say = fn != nullptr;
#define ROWS_REQUIRE(cond, code, ...)                \
    do {                                             \
        if (!(cond)) {                               \
            if (say) rtk_set_error(__VA_ARGS__);     \
            return (code);                           \
        }                                            \
    } while (0)
    ROWS_REQUIRE(batch < (1ll << 31) - 32 && (int64_t)b * (32 * ((int64_t)a / 32 + 1)) < (1ll << 31) - 64, RTK_ERR_UNSUPPORTED,
                 "%s: dimension too large", fn);
    ROWS_REQUIRE(c <= 16 * SW_MAX_KS_F32, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d (the ws kernel's range)", fn, c,
                 16 * SW_MAX_KS_F32);
    ROWS_REQUIRE(c % 4 == 0 && (reinterpret_cast<uintptr_t>(core) & 15) == 0, RTK_ERR_UNSUPPORTED,
                 "%s: fp32 needs c %% 4 == 0 and a 16-byte-aligned core (c = %d)", fn, c);
#undef ROWS_REQUIRE
    return RTK_OK;
}

// ---- the core gradient ---------------------------------------------------------------------------------------------
// Tile 32 (m = i b + j) x 128 (k of the core), k-tiles of 16 queries; 4 waves, wave w owns columns 32 w .. 32 w + 31 and
// all of them share the A fragment.  Both operands lie in LDS [query][row] as in rtk_gemm_f32.hip.
constexpr int OBM = 32, OBN = 128, OBK = 16, OLDA = 36, OLDB = 132;

__global__ __launch_bounds__(256) void core_outer_kernel(const float *__restrict__ x, int64_t ld_x,
                                                         const float *__restrict__ y, int64_t ld_y, int b,
                                                         const float *__restrict__ z, int64_t ld_z, bool z_vec, int M, int N,
                                                         int K, int n_tn, float *__restrict__ gG) {
    __shared__ __attribute__((aligned(16))) float As[OBK * OLDA];
    __shared__ __attribute__((aligned(16))) float Bs[OBK * OLDB];
    const int tile_m = ((int)blockIdx.x / n_tn) * OBM, tile_n = ((int)blockIdx.x % n_tn) * OBN;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;

    // A: thread t stages element m = t & 31 of queries k0 + (t >> 5) and k0 + 8 + (t >> 5): one fp32 product each
    const int am = tile_m + (t & 31), ak = t >> 5;
    const bool a_in = am < M;
    const int ai = a_in ? am / b : 0, aj = a_in ? am - ai * b : 0;
    // B: thread t stages columns 8 (t & 15) .. + 7 of query k0 + (t >> 4)
    const int bk = t >> 4, bn = tile_n + 8 * (t & 15);
    float sa[2], sb[8];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t d = k0 + ak + 8 * q;
            sa[q] = (a_in && d < K) ? __fmul_rn(x[d * ld_x + ai], y[d * ld_y + aj]) : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) sb[q] = 0.f;
        const int64_t d = k0 + bk;
        if (d < K) {
            const float *p = z + d * ld_z + bn;
            if (z_vec && bn + 8 <= N) {
                const f32x4 x0 = rtk_load4(p), x1 = rtk_load4(p + 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    sb[q] = x0[q];
                    sb[4 + q] = x1[q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (bn + q < N) sb[q] = p[q];
            }
        }
    };
    auto stash = [&]() {
        As[ak * OLDA + (t & 31)] = sa[0];
        As[(ak + 8) * OLDA + (t & 31)] = sa[1];
        *reinterpret_cast<f32x4 *>(&Bs[bk * OLDB + 8 * (t & 15)]) = f32x4{sb[0], sb[1], sb[2], sb[3]};
        *reinterpret_cast<f32x4 *>(&Bs[bk * OLDB + 8 * (t & 15) + 4]) = f32x4{sb[4], sb[5], sb[6], sb[7]};
    };

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    load(0);
    stash();
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += OBK) {
        const bool more = k0 + OBK < K;
        if (more) load(k0 + OBK);
#pragma unroll
        for (int ks = 0; ks < OBK / 2; ++ks) {
            const int kk = 2 * ks + h;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk * OLDA + r], Bs[kk * OLDB + wave * 32 + r], acc, 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            stash();
            __syncthreads();
        }
    }
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    const int n = tile_n + wave * 32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = tile_m + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (m < M && n < N) gG[(int64_t)m * N + n] = acc[e];
    }
}

// ---- the row scatter's entries: entity idx[d] (outside [0, n_out): none), owner d, factor 1 ------------------------
__global__ __launch_bounds__(256) void rows_entries_kernel(const int64_t *__restrict__ idx, int64_t B, int64_t n_out,
                                                           int32_t *__restrict__ ent, int32_t *__restrict__ owner,
                                                           float *__restrict__ one) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < B; d += (int64_t)gridDim.x * 256) {
        const int64_t e = idx[d];
        ent[d] = e >= 0 && e < n_out ? (int32_t)e : -1;
        owner[d] = (int32_t)d;
        one[d] = 1.0f;
    }
}

size_t scatter_rows_lists(int64_t batch) { return rtk_align_up((size_t)batch * 4, 256); }

}  // namespace

extern "C" size_t rtk_pair_rows_workspace_bytes(int64_t batch, int a, int b, int c) {
    if (batch <= 0 || a < 1 || b < 1 || c < 1) return 0;
    // (the alignment of the core is the call's to check)
    return rows_check_shape(nullptr, batch, a, b, c, nullptr) == RTK_OK ? rows_layout(batch, a, b, c).total : 0;
}

extern "C" int rtk_pair_rows_f32(const float *core, int a, int b, int c, const float *X, int64_t n_x, const int64_t *x_idx,
                                 const float *w, int64_t ld_w, int64_t batch, float *rows, int64_t ld_rows, void *workspace,
                                 size_t ws_bytes, void *stream) {
    const char *fn = "rtk_pair_rows_f32";
    RTK_REQUIRE(core && X, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(batch >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld must be >= 0", fn, (long long)batch);
    RTK_REQUIRE(a >= 1 && b >= 1 && c >= 1 && n_x >= 1, RTK_ERR_BAD_ARG, "%s: sizes must be positive (a=%d b=%d c=%d n_x=%lld)",
                fn, a, b, c, (long long)n_x);
    RTK_REQUIRE(ld_w >= a, RTK_ERR_BAD_ARG, "%s: ld_w = %lld below a = %d", fn, (long long)ld_w, a);
    RTK_REQUIRE(ld_rows >= b, RTK_ERR_BAD_ARG, "%s: ld_rows = %lld below b = %d", fn, (long long)ld_rows, b);
    const int rc = rows_check_shape(fn, batch, a, b, c, core);
    if (rc != RTK_OK) return rc;
    if (batch == 0) return RTK_OK;
    RTK_REQUIRE(x_idx && w && rows, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    const RowsLayout L = rows_layout(batch, a, b, c);
    RTK_REQUIRE(workspace && ws_bytes >= L.total, RTK_ERR_WORKSPACE, "%s: workspace of %zu bytes given, %zu needed", fn,
                workspace ? ws_bytes : (size_t)0, L.total);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned",
                fn);

    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    unsigned char *planes = ws + L.planes;
    float *wg = reinterpret_cast<float *>(ws + L.wg), *part = reinterpret_cast<float *>(ws + L.part);
    const int B = (int)batch, ks = (c + 15) / 16;
    hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)(L.n_mt * 32)), dim3(256), 0, st, X, n_x, x_idx, w, ld_w, B, a,
                       L.a_pad, c, ks, planes, wg, reinterpret_cast<uint32_t *>(ws));
    const SweepGrid g = grid_of(batch, L.n_rows, SW_SLOTS);
    const int rcl = rtk_dispatch_ksteps<SW_MAX_KS_F32>(ks, fn, [&](auto K) {
        return launch_lds<&rows_kernel<K.value>, 2 * (int)tile_bytes<float, K.value>()>(
            dim3((unsigned)(g.n_slots * g.qsplit)), dim3(64 * SW_WAVES), st, fn, (const unsigned char *)planes, B, core,
            (int)L.n_rows, c, a, b, L.a_pad, (const float *)wg, part, g.n_slots, g.qsplit);
    });
    if (rcl != RTK_OK) return rcl;
    hipLaunchKernelGGL(rows_finish_kernel, dim3((unsigned)L.n_mt, (unsigned)rtk_cdiv(b, 8)), dim3(256), 0, st,
                       (const float *)part, B, b, L.na, rows, ld_rows);
    return rtk_check_launch(fn);
}

extern "C" int rtk_core_outer_f32(const float *x, int64_t ld_x, int a, const float *y, int64_t ld_y, int b, const float *z,
                                  int64_t ld_z, int c, int64_t batch, float *gG, void *stream) {
    const char *fn = "rtk_core_outer_f32";
    RTK_REQUIRE(gG, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(a >= 1 && b >= 1 && c >= 1 && batch >= 0, RTK_ERR_BAD_ARG, "%s: sizes must be positive (a=%d b=%d c=%d batch=%lld)",
                fn, a, b, c, (long long)batch);
    RTK_REQUIRE(ld_x >= a && ld_y >= b && ld_z >= c, RTK_ERR_BAD_ARG,
                "%s: pitches ld_x = %lld, ld_y = %lld, ld_z = %lld below the widths a = %d, b = %d, c = %d", fn, (long long)ld_x,
                (long long)ld_y, (long long)ld_z, a, b, c);
    RTK_REQUIRE((int64_t)a * b * c < (1ll << 31) && (int64_t)a * b < (1ll << 31) && batch < (1ll << 31) - OBK, RTK_ERR_UNSUPPORTED,
                "%s: dimension too large", fn);
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0) return rtk_zero_async(fn, gG, (size_t)a * b * c * 4, st);
    RTK_REQUIRE(x && y && z, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    const int M = a * b, n_tn = (int)rtk_cdiv(c, OBN);
    const bool z_vec = (reinterpret_cast<uintptr_t>(z) & 15) == 0 && ld_z % 4 == 0;
    hipLaunchKernelGGL(core_outer_kernel, dim3((unsigned)(rtk_cdiv(M, OBM) * n_tn)), dim3(256), 0, st, x, ld_x, y, ld_y, b, z,
                       ld_z, z_vec, M, c, (int)batch, n_tn, gG);
    return rtk_check_launch(fn);
}

extern "C" size_t rtk_scatter_rows_workspace_bytes(int64_t batch) {
    if (batch <= 0 || batch >= (1ll << 31)) return 0;
    return 3 * scatter_rows_lists(batch) + rtk_scatter_bytes(batch);
}

extern "C" int rtk_scatter_rows_f32(const int64_t *idx, const float *rows, int64_t ld_rows, int64_t batch, int n, int64_t n_out,
                                    float *out, void *workspace, size_t ws_bytes, void *stream) {
    const char *fn = "rtk_scatter_rows_f32";
    RTK_REQUIRE(out, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(batch >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld must be >= 0", fn, (long long)batch);
    RTK_REQUIRE(n >= 1 && n_out >= 1, RTK_ERR_BAD_ARG, "%s: sizes must be positive (n=%d n_out=%lld)", fn, n, (long long)n_out);
    RTK_REQUIRE(ld_rows >= n, RTK_ERR_BAD_ARG, "%s: ld_rows = %lld below n = %d", fn, (long long)ld_rows, n);
    RTK_REQUIRE(n <= RTK_SCATTER_MAXC, RTK_ERR_UNSUPPORTED, "%s: n = %d above %d", fn, n, RTK_SCATTER_MAXC);
    RTK_REQUIRE(batch < (1ll << 31) && n_out < (1ll << 31) - 1, RTK_ERR_UNSUPPORTED, "%s: dimension too large", fn);
    hipStream_t st = (hipStream_t)stream;
    if (batch == 0) return rtk_zero_async(fn, out, (size_t)n_out * n * 4, st);
    RTK_REQUIRE(idx && rows, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    const size_t need = rtk_scatter_rows_workspace_bytes(batch);
    RTK_REQUIRE(workspace && ws_bytes >= need, RTK_ERR_WORKSPACE, "%s: workspace of %zu bytes given, %zu needed", fn,
                workspace ? ws_bytes : (size_t)0, need);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned",
                fn);
    unsigned char *ws = (unsigned char *)workspace;
    const size_t ll = scatter_rows_lists(batch);
    int32_t *ent = reinterpret_cast<int32_t *>(ws), *owner = reinterpret_cast<int32_t *>(ws + ll);
    float *one = reinterpret_cast<float *>(ws + 2 * ll);
    const int64_t blocks = rtk_cdiv(batch, 256);
    hipLaunchKernelGGL(rows_entries_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, idx, batch, n_out,
                       ent, owner, one);
    return rtk_scatter_flat_ld(fn, ent, owner, one, batch, n_out, rows, ld_rows, n, out, ws + 3 * ll, st);
}
