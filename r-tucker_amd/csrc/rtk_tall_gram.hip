// C = A^T B of two tall fp32 blocks, every product and every sum in float64, on the f64 matrix pipe: rtk_tall_gram_f64.
//
// The Cholesky-QR rounds of the Riemannian step (r-tucker_amd/tucker.py::_orth_tall_many) need the Gram matrix of a
// tall block positive semi-definite to well below their diagonal shift, so it is accumulated in float64
// (smalllinalg.tall_gram_f64: the fp32 Gram kernel's noise over 40 943 rows made it indefinite).
// The torch form of that product writes a zero-padded float64 copy of the block (n x k x 8 bytes: 512 MB for a
// 125 000 x 512 entity shard) and runs a batched float64 rocBLAS product on it.  Here the fp32 rows are read as they
// are -- through a row pitch, so the two column halves of an n x 2k matrix are operands without a copy -- converted
// in registers (v_cvt_f64_f32: exact) and multiplied by v_mfma_f64_16x16x4_f64; the product of two fp32 values is
// exact in float64, so the only roundings are those of the float64 additions.
//
// Tiling.  One 256-thread workgroup owns a 64 x 64 tile of C and one RANGE of rows.  It stages 32 rows x 64 columns
// of A and of B in LDS as fp32 (16-byte loads when both bases and pitches are 16-byte aligned and p % 4 == q % 4 == 0,
// element loads otherwise; the next chunk's loads are in flight while the current one is multiplied; rows at or
// beyond the end of the range and columns beyond p / q are staged as zeros and never read), and each of its four
// waves keeps a 32 x 32 sub-tile in four accumulators: eight k-steps of four rows per chunk.  Lane l = (i = l & 15,
// k = l >> 4) supplies A[row k][column i] and B[row k][column i] of a k-step; accumulator element e is row
// (l >> 4) + 4 e, column l & 15 of the 16 x 16 result.  The LDS rows are 80 floats apart, so the two rows that one
// half-wave reads fall on disjoint banks.
//
// Summation order.  The rows are cut into `ranges` equal ranges (the last may be short), a function of (n, p, q)
// only (tall_gram_split below).  Within a range an output element is one chain over the rows in ascending order, four
// rows per instruction.  Every range's partial matrix goes to the workspace, and a second launch adds the partials
// in range order from zero.  No atomics: repeated calls give the same bits; two launches, always, no host
// synchronisation.  n == 0 runs the same two launches on an empty range and writes zeros.
#include "rtk_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 64;          // a workgroup's tile of C is TILE x TILE
constexpr int KC = 32;            // rows staged per chunk
constexpr int LDP = TILE + 16;    // LDS row pitch in floats
constexpr int NT = 256;
constexpr int PQ_MAX = 1024;
constexpr int64_t MIN_ROWS = 1024;            // shortest range (a multiple of KC)
constexpr int64_t TARGET_WG = 1024;           // workgroups aimed at (four per CU)
constexpr size_t WS_MAX = (size_t)64 << 20;   // the partials never take more

struct Split {
    int64_t len;      // rows per range, a multiple of KC
    int ranges;       // >= 1
};

// The static split rule: as many ranges as it takes to reach TARGET_WG workgroups, no more than fit the workspace cap,
// none shorter than MIN_ROWS.
Split tall_gram_split(int64_t n, int p, int q) {
    const int64_t tiles = rtk_cdiv(p, TILE) * rtk_cdiv(q, TILE);
    int64_t smax = TARGET_WG / tiles;
    const int64_t cap = (int64_t)(WS_MAX / ((size_t)p * q * sizeof(double)));
    if (smax > cap) smax = cap;
    if (smax < 1) smax = 1;
    int64_t len = rtk_cdiv(n, smax);
    if (len < MIN_ROWS) len = MIN_ROWS;
    len = rtk_cdiv(len, KC) * KC;
    int64_t ranges = rtk_cdiv(n, len);
    if (ranges < 1) ranges = 1;
    return Split{len, (int)ranges};
}

// 32 rows x 64 columns of one operand, from row r of the range: this thread's share into registers.
// VEC: two 16-byte pieces (chunk id t and t + 256 of 32 x 16); otherwise eight elements (id t + 256 u of 32 x 64).
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float *__restrict__ X, int64_t ld, int cols, int c0, int64_t r,
                                           int64_t r1, int t, f32x4 (&v)[2]) {
    if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int id = t + u * NT, row = id >> 4, c = c0 + ((id & 15) << 2);
            v[u] = (r + row < r1 && c < cols) ? *reinterpret_cast<const f32x4 *>(X + (r + row) * ld + c)
                                              : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int id = t + u * NT, row = id >> 6, c = c0 + (id & 63);
            v[u >> 2][u & 3] = (r + row < r1 && c < cols) ? X[(r + row) * ld + c] : 0.f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_chunk(float (*s)[LDP], int t, const f32x4 (&v)[2]) {
    if constexpr (VEC) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int id = t + u * NT;
            *reinterpret_cast<f32x4 *>(&s[id >> 4][(id & 15) << 2]) = v[u];
        }
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int id = t + u * NT;
            s[id >> 6][id & 63] = v[u >> 2][u & 3];
        }
    }
}

// grid (tiles, ranges): partial[range][i][j] = sum over the range's rows of A[k, i] * B[k, j]
template <bool VEC>
__global__ __launch_bounds__(NT) void tall_gram_partial_kernel(const float *__restrict__ A, int64_t lda,
                                                               const float *__restrict__ B, int64_t ldb, int64_t n, int p,
                                                               int q, int64_t len, int tiles_q, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sa[KC][LDP];
    __shared__ __attribute__((aligned(16))) float sb[KC][LDP];
    const int t = threadIdx.x;
    const int tile = blockIdx.x, i0 = (tile / tiles_q) * TILE, j0 = (tile % tiles_q) * TILE;
    const int64_t r0 = (int64_t)blockIdx.y * len;
    const int64_t r1 = r0 + len < n ? r0 + len : n;
    const int lane = t & 63, wv = t >> 6, li = lane & 15, lq = lane >> 4;
    const int wi = (wv >> 1) * 32, wj = (wv & 1) * 32;      // the wave's 32 x 32 sub-tile
    const bool live = i0 + wi < p && j0 + wj < q;           // wave-uniform: a sub-tile wholly outside C multiplies nothing
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};
    f32x4 va[2], vb[2];
    if (r0 < r1) {
        load_chunk<VEC>(A, lda, p, i0, r0, r1, t, va);
        load_chunk<VEC>(B, ldb, q, j0, r0, r1, t, vb);
    }
    for (int64_t r = r0; r < r1; r += KC) {
        __syncthreads();                                    // the previous chunk has been multiplied
        store_chunk<VEC>(sa, t, va);
        store_chunk<VEC>(sb, t, vb);
        __syncthreads();
        if (r + KC < r1) {
            load_chunk<VEC>(A, lda, p, i0, r + KC, r1, t, va);
            load_chunk<VEC>(B, ldb, q, j0, r + KC, r1, t, vb);
        }
        if (live) {
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                const double a0 = (double)sa[4 * kk + lq][wi + li], a1 = (double)sa[4 * kk + lq][wi + 16 + li];
                const double b0 = (double)sb[4 * kk + lq][wj + li], b1 = (double)sb[4 * kk + lq][wj + 16 + li];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    double *out = part + (size_t)blockIdx.y * p * q;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + wi + 16 * x + lq + 4 * e, j = j0 + wj + 16 * y + li;
                if (i < p && j < q) out[(size_t)i * q + j] = acc[x][y][e];
            }
}

// C[e] = part[0][e] + part[1][e] + ... in range order, from zero
__global__ __launch_bounds__(NT) void tall_gram_sum_kernel(const double *__restrict__ part, int ranges, int64_t pq,
                                                           double *__restrict__ C) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= pq) return;
    double s = 0.0;
    int r = 0;
    for (; r + 4 <= ranges; r += 4) {                       // four loads in flight, added in order
        const double x0 = part[(size_t)r * pq + e], x1 = part[(size_t)(r + 1) * pq + e];
        const double x2 = part[(size_t)(r + 2) * pq + e], x3 = part[(size_t)(r + 3) * pq + e];
        s += x0; s += x1; s += x2; s += x3;
    }
    for (; r < ranges; ++r) s += part[(size_t)r * pq + e];
    C[e] = s;
}

bool covered(int p, int q) { return p >= 1 && p <= PQ_MAX && q >= 1 && q <= PQ_MAX; }

}  // namespace

extern "C" size_t rtk_tall_gram_f64_workspace_bytes(int64_t n, int p, int q) {
    if (n < 0 || !covered(p, q)) return 0;
    return rtk_align_up((size_t)tall_gram_split(n, p, q).ranges * p * q * sizeof(double), 256);
}

extern "C" int rtk_tall_gram_f64(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t n, int p, int q,
                                 double *C, void *workspace, size_t ws_bytes, void *stream) {
    RTK_REQUIRE(A && B && C && workspace, RTK_ERR_BAD_ARG, "rtk_tall_gram_f64: null operand");
    RTK_REQUIRE(n >= 0, RTK_ERR_BAD_ARG, "rtk_tall_gram_f64: n=%lld must be >= 0", (long long)n);
    RTK_REQUIRE(covered(p, q), RTK_ERR_UNSUPPORTED, "rtk_tall_gram_f64: p=%d, q=%d not in [1, %d]", p, q, PQ_MAX);
    RTK_REQUIRE(lda >= p && ldb >= q, RTK_ERR_BAD_ARG, "rtk_tall_gram_f64: pitch lda=%lld, ldb=%lld below p=%d, q=%d",
                (long long)lda, (long long)ldb, p, q);
    const size_t need = rtk_tall_gram_f64_workspace_bytes(n, p, q);
    RTK_REQUIRE(ws_bytes >= need, RTK_ERR_BAD_ARG, "rtk_tall_gram_f64: workspace of %zu bytes given, %zu needed", ws_bytes,
                need);
    RTK_REQUIRE(((uintptr_t)workspace & 255) == 0, RTK_ERR_BAD_ARG, "rtk_tall_gram_f64: workspace must be 256-byte aligned");
    const Split sp = tall_gram_split(n, p, q);
    const int tiles_q = (int)rtk_cdiv(q, TILE);
    const dim3 grid((unsigned)(rtk_cdiv(p, TILE) * tiles_q), (unsigned)sp.ranges);
    const bool vec = (((uintptr_t)A | (uintptr_t)B) & 15) == 0 && lda % 4 == 0 && ldb % 4 == 0 && p % 4 == 0 && q % 4 == 0;
    const hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    if (vec)
        hipLaunchKernelGGL(tall_gram_partial_kernel<true>, grid, dim3(NT), 0, st, A, lda, B, ldb, n, p, q, sp.len, tiles_q, part);
    else
        hipLaunchKernelGGL(tall_gram_partial_kernel<false>, grid, dim3(NT), 0, st, A, lda, B, ldb, n, p, q, sp.len, tiles_q, part);
    const int rc = rtk_check_launch("rtk_tall_gram_f64");
    if (rc != RTK_OK) return rc;
    const int64_t pq = (int64_t)p * q;
    hipLaunchKernelGGL(tall_gram_sum_kernel, dim3((unsigned)rtk_cdiv(pq, NT)), dim3(NT), 0, st, (const double *)part,
                       sp.ranges, pq, C);
    return rtk_check_launch("rtk_tall_gram_f64");
}
