// Relation prediction, stage 1: the "pair vectors" of (h, ?, t) queries without the (B, a*b) intermediate.
//
//   W[d, i, j] = sum_k G[i, j, k] * O[t_d, k]       the score GEMM with the core, a row-major (a*b, c) matrix, in O's place
//   u[d, i]    = sum_j S[h_d, j] * W[d, i, j]       (B, a) fp32;  z = u . R^T is an ordinary stage 2 (rtk_score_packed_*)
//
// Three launches on the caller's stream:
//
//   gather_kernel    one workgroup per row of the query tiles: checks and clamps t_d and h_d (error word: 4 for an
//                    object id, 1 for a subject id), writes the packed planes of O[t_d] -- the layout and the bits
//                    rtk_pack_query_vectors gives for these rows; bf16 rows are copied, not rounded -- and S[h_d] as
//                    fp32, zero-padded to b_pad columns.  Rows past the batch in the last tile are zeros.
//   pair_kernel      the entity-stationary sweep (rtk_score_rank_kernel.h) with the core's rows as the "entities".
//                    Rows are indexed i * b_pad + j, b_pad = 32 ceil(b / 32): the 32 rows of a wave (one "chunk")
//                    belong to ONE i, the padding rows j >= b re-read row b - 1 and contribute 0.  A lane holds one
//                    row (i, j) and 16 queries: acc * (row factor * column factor) is the logit-scale W[d, i, j], times
//                    S[h_d, j] (read from the gathered rows, 32 consecutive floats per half wave), summed over the 32
//                    lanes by reduce16 and stored as the chunk's partial sum, part[mt][chunk][32 queries].  Nothing
//                    else is written: B * a * b_pad / 32 floats.
//   finish_kernel    u[d, i] = the b_pad / 32 partials of (d, i) added in ascending chunk order; pack_u_kernel then
//                    writes the packed planes of u when asked for.
//
// The bits of u[d, :] depend only on O[t_d], S[h_d], the core and the operand type.  An MFMA output element does not
// depend on its place in the tile, the planes' row factor is per query, reduce16 combines the 32 lanes of a chunk in one
// fixed tree whatever the element, every (query, chunk) partial has exactly one writer whatever the grid (qsplit only
// deals query tiles to workgroups), and finish_kernel adds a query's partials in one order.  No atomics on data.
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_rank_kernel.h"

namespace {

constexpr int PAIR_MAX_A_PACKED = 512;         // the packed planes of u: rtk_pack_query_vectors' range

__device__ __forceinline__ int64_t clamp_id(int64_t x, int64_t n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

// the largest of the workgroup's (256 threads) values, in every thread
__device__ __forceinline__ float block_max(float mx, float *red, int t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

template <typename T>
__global__ __launch_bounds__(256) void gather_kernel(const T *__restrict__ S, int64_t n_subj, const T *__restrict__ O,
                                                     int64_t n_obj, const int64_t *__restrict__ subject_idx,
                                                     const int64_t *__restrict__ object_idx, int B, int b, int b_pad,
                                                     int c, int ksteps, unsigned char *__restrict__ planes,
                                                     float *__restrict__ sg, uint32_t *__restrict__ err) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const int64_t d = blockIdx.x;
    const bool live = d < B;                                          // workgroup-uniform
    int64_t hh = 0, tt = 0;
    if (live) {
        const int64_t h_raw = subject_idx[d], t_raw = object_idx[d];
        hh = clamp_id(h_raw, n_subj);
        tt = clamp_id(t_raw, n_obj);
        if (t == 0 && hh != h_raw) atomicOr(err, 1u);
        if (t == 0 && tt != t_raw) atomicOr(err, 4u);
    }
    const T *srow = S + hh * b;
    for (int j = t; j < b_pad; j += 256) sg[d * b_pad + j] = (live && j < b) ? rtk_to_f32(srow[j]) : 0.f;
    const T *orow = O + tt * c;
    const int cl = live ? c : 0;                                      // a row past the batch: zeros
    if constexpr (sizeof(T) == 4) {
        float mx = 0.f;
        for (int k = t; k < cl; k += 256) mx = fmaxf(mx, fabsf(orow[k]));
        rtk_pack_store_row_f32(planes, d, ksteps, orow, cl, block_max(mx, red, t), t, 256);
    } else {
        rtk_pack_store_row_bf16(planes, d, ksteps, t, 256, [=](int k) { return k < cl ? orow[k] : (rtk_bf16)0; });
    }
}

// What pair_kernel does with the sweep: nothing travels with a query tile; the 32 x 32 accumulators become a chunk's
// partial sums.
template <typename T, int KS>
struct PairSweep {
    static constexpr int EXTRA = 0;
    int b, b_pad, nb, n_chunks;                    // nb = b_pad / 32 chunks per i, n_chunks = a * nb
    const float *__restrict__ sg;                  // (32 n_mt, b_pad): S[h_d] as fp32, zero-padded
    float *__restrict__ part;                      // (n_mt, n_chunks, 32)

    __device__ __forceinline__ void load_extra(SweepLane, int) const {}
    __device__ __forceinline__ void store_extra(SweepLane, int) const {}
    __device__ __forceinline__ void begin_tile() const {}
    __device__ __forceinline__ void end_tile(SweepLane, int) const {}
    __device__ __forceinline__ void publish(SweepLane, int, int, int, int, int, bool) const {}
    // row i * b_pad + j of the sweep reads row i * b + min(j, b - 1) of the core
    __device__ __forceinline__ int64_t row_of(int jl) const {
        const int i = jl / b_pad, j = jl - i * b_pad;
        return (int64_t)i * b + min(j, b - 1);
    }
    __device__ __forceinline__ void score(SweepLane ln, const Frag<T, KS> &f, const f32x16 &acc,
                                          const unsigned char *buf, int, int jl, bool, int mt) const {
        const int r = ln.r, h = ln.h;
        const int chunk = __builtin_amdgcn_readfirstlane(jl >> 5);    // the wave's 32 rows: one i, columns 32 jc + r
        if (chunk >= n_chunks) return;                                // (wave-uniform) past the last row: the rows come in 32s
        const int j = (chunk % nb) * 32 + r;
        const bool live = j < b;
        const float *sq = sg + (int64_t)mt * 32 * b_pad + j;
        float v[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rw = acc_row(4 * g, h);
            f32x4 sr4 = {1.f, 1.f, 1.f, 1.f};
            if constexpr (Frag<T, KS>::PLANES == 2) sr4 = *reinterpret_cast<const f32x4 *>(buf + rw * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                const float s = sq[(int64_t)(rw + q) * b_pad];
                float w = acc[e];
                if constexpr (Frag<T, KS>::PLANES == 2) w = w * (sr4[q] * f.kcol);
                v[e] = live ? w * s : 0.f;
            }
        }
        const float sum = reduce16(v, r, RedSum());
        if (!(r & 1)) part[((int64_t)mt * n_chunks + chunk) * 32 + red_row(r, h)] = sum;
    }
};

template <typename T, int KS>
__global__ __launch_bounds__(64 * SW_WAVES, 2) void pair_kernel(const unsigned char *__restrict__ planes, int B,
                                                                const T *__restrict__ core, int n_rows, int c, int b,
                                                                int b_pad, const float *__restrict__ sg,
                                                                float *__restrict__ part, int n_slots, int qsplit, bool vec) {
    const int nb = b_pad >> 5;
    PairSweep<T, KS> pol{b, b_pad, nb, n_rows >> 5, sg, part};
    sweep<T, KS, 1>(pol, planes, B, core, n_rows, c, vec, n_slots, qsplit);
}

// u[d, i] = sum of the nb partials of (d, i), ascending.  Workgroup (mt, y): the 32 queries of tile mt, i = 8 y .. 8 y + 7.
__global__ __launch_bounds__(256) void finish_kernel(const float *__restrict__ part, int B, int a, int nb,
                                                     float *__restrict__ u, int64_t ld_u) {
    const int t = threadIdx.x, rw = t & 31, i = (int)blockIdx.y * 8 + (t >> 5);
    const int mt = blockIdx.x, d = mt * 32 + rw;
    if (i >= a || d >= B) return;
    const float *p = part + (((int64_t)mt * a + i) * nb) * 32 + rw;
    float s = p[0];
    for (int jc = 1; jc < nb; ++jc) s += p[(int64_t)jc * 32];
    u[d * ld_u + i] = s;
}

// the packed planes of u (rtk_pack_query_vectors' rows, from a pitched u)
template <bool BF16>
__global__ __launch_bounds__(256) void pack_u_kernel(const float *__restrict__ u, int64_t ld_u, int a, int ksteps,
                                                     unsigned char *__restrict__ packed) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const int64_t d = blockIdx.x;
    const float *row = u + d * ld_u;
    if (BF16) {
        rtk_pack_store_row_bf16(packed, d, ksteps, row, a, t, 256);
        return;
    }
    float mx = 0.f;
    for (int k = t; k < a; k += 256) mx = fmaxf(mx, fabsf(row[k]));
    rtk_pack_store_row_f32(packed, d, ksteps, row, a, block_max(mx, red, t), t, 256);
}

// workspace: the error word's header, the planes of O[t], the gathered S rows, the chunk partials
struct PairLayout {
    int b_pad, nb;
    int64_t n_mt, n_rows;
    size_t planes, sg, part, total;
};
PairLayout layout_of(int dtype, int64_t batch, int a, int b, int c) {
    PairLayout L;
    L.nb = (b + 31) / 32;
    L.b_pad = 32 * L.nb;
    L.n_mt = rtk_cdiv(batch, 32);
    L.n_rows = (int64_t)a * L.b_pad;
    L.planes = 256;
    L.sg = L.planes + rtk_align_up((size_t)L.n_mt * (size_t)rtk_pack_tile_bytes((c + 15) / 16, dtype == RTK_F32 ? 2 : 1), 256);
    L.part = L.sg + rtk_align_up((size_t)L.n_mt * 32 * L.b_pad * 4, 256);
    L.total = L.part + rtk_align_up((size_t)L.n_mt * (size_t)a * L.nb * 32 * 4, 256);
    return L;
}

// the shapes the sweep covers; fn == nullptr: only asked (no message)
template <typename T>
int check_shape(const char *fn, int64_t batch, int a, int b, int c, const void *core) {
    const bool say = fn != nullptr;
#define PAIR_REQUIRE(cond, code, ...)                \
    do {                                             \
        if (!(cond)) {                               \
            if (say) rtk_set_error(__VA_ARGS__);     \
            return (code);                           \
        }                                            \
    } while (0)
    PAIR_REQUIRE(batch < (1ll << 31) - 32 && (int64_t)a * (32 * ((int64_t)b / 32 + 1)) < (1ll << 31) - 64, RTK_ERR_UNSUPPORTED,
                 "%s: dimension too large", fn);
    if (sizeof(T) == 4) {
        PAIR_REQUIRE(c <= 16 * SW_MAX_KS_F32, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d (the ws kernel's range)", fn, c,
                     16 * SW_MAX_KS_F32);
        PAIR_REQUIRE(c % 4 == 0 && (reinterpret_cast<uintptr_t>(core) & 15) == 0, RTK_ERR_UNSUPPORTED,
                     "%s: fp32 needs c %% 4 == 0 and a 16-byte-aligned core (c = %d)", fn, c);
    } else {
        PAIR_REQUIRE(c <= 16 * SW_MAX_KS_BF16, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d", fn, c, 16 * SW_MAX_KS_BF16);
    }
#undef PAIR_REQUIRE
    return RTK_OK;
}

template <typename T>
int pair_vectors(const char *fn, const T *core, int a, int b, int c, const T *S, int64_t n_subj, const T *O, int64_t n_obj,
                 const int64_t *subject_idx, const int64_t *object_idx, int64_t batch, float *u, int64_t ld_u,
                 void *packed_u, void *workspace, size_t ws_bytes, void *stream) {
    constexpr int dtype = sizeof(T) == 4 ? RTK_F32 : RTK_BF16;
    RTK_REQUIRE(core && S && O, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(batch >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld must be >= 0", fn, (long long)batch);
    RTK_REQUIRE(a >= 1 && b >= 1 && c >= 1 && n_subj >= 1 && n_obj >= 1, RTK_ERR_BAD_ARG,
                "%s: sizes must be positive (a=%d b=%d c=%d n_subj=%lld n_obj=%lld)", fn, a, b, c, (long long)n_subj,
                (long long)n_obj);
    RTK_REQUIRE(ld_u >= a, RTK_ERR_BAD_ARG, "%s: ld_u = %lld below a = %d", fn, (long long)ld_u, a);
    const int rc = check_shape<T>(fn, batch, a, b, c, core);
    if (rc != RTK_OK) return rc;
    RTK_REQUIRE(!packed_u || a <= PAIR_MAX_A_PACKED, RTK_ERR_UNSUPPORTED,
                "%s: packed planes of u need a <= %d (a = %d): pass packed_u = NULL and score u with rtk_score_f32", fn,
                PAIR_MAX_A_PACKED, a);
    if (batch == 0) return RTK_OK;
    RTK_REQUIRE(subject_idx && object_idx && u, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    const PairLayout L = layout_of(dtype, batch, a, b, c);
    RTK_REQUIRE(workspace && ws_bytes >= L.total, RTK_ERR_WORKSPACE, "%s: workspace of %zu bytes given, %zu needed", fn,
                workspace ? ws_bytes : (size_t)0, L.total);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned",
                fn);

    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    unsigned char *planes = ws + L.planes;
    float *sg = reinterpret_cast<float *>(ws + L.sg), *part = reinterpret_cast<float *>(ws + L.part);
    const int B = (int)batch, ks = (c + 15) / 16;
    hipLaunchKernelGGL(gather_kernel<T>, dim3((unsigned)(L.n_mt * 32)), dim3(256), 0, st, S, n_subj, O, n_obj, subject_idx,
                       object_idx, B, b, L.b_pad, c, ks, planes, sg, reinterpret_cast<uint32_t *>(ws));
    const SweepGrid g = grid_of(batch, L.n_rows, SW_SLOTS);
    const bool vec = vec_rows(core, c);
    int rcl = rtk_dispatch_ksteps<sizeof(T) == 4 ? SW_MAX_KS_F32 : SW_MAX_KS_BF16>(ks, fn, [&](auto K) {
        return launch_lds<&pair_kernel<T, K.value>, 2 * (int)tile_bytes<T, K.value>()>(
            dim3((unsigned)(g.n_slots * g.qsplit)), dim3(64 * SW_WAVES), st, fn, (const unsigned char *)planes, B, core,
            (int)L.n_rows, c, b, L.b_pad, (const float *)sg, part, g.n_slots, g.qsplit, vec);
    });
    if (rcl != RTK_OK) return rcl;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)L.n_mt, (unsigned)rtk_cdiv(a, 8)), dim3(256), 0, st, (const float *)part, B,
                       a, L.nb, u, ld_u);
    if (packed_u) {
        const int ksa = (a + 15) / 16;
        hipLaunchKernelGGL(pack_u_kernel<sizeof(T) == 2>, dim3((unsigned)B), dim3(256), 0, st, (const float *)u, ld_u, a, ksa,
                           (unsigned char *)packed_u);
    }
    return rtk_check_launch(fn);
}

}  // namespace

extern "C" size_t rtk_pair_vectors_workspace_bytes(int dtype, int64_t batch, int a, int b, int c) {
    if (batch <= 0 || a < 1 || b < 1 || c < 1 || (dtype != RTK_F32 && dtype != RTK_BF16)) return 0;
    // (the alignment of the core is the call's to check)
    const int rc = dtype == RTK_F32 ? check_shape<float>(nullptr, batch, a, b, c, nullptr)
                                    : check_shape<rtk_bf16>(nullptr, batch, a, b, c, nullptr);
    return rc == RTK_OK ? layout_of(dtype, batch, a, b, c).total : 0;
}

extern "C" int rtk_pair_vectors_f32(const float *core, int a, int b, int c, const float *S, int64_t n_subj, const float *O,
                                    int64_t n_obj, const int64_t *subject_idx, const int64_t *object_idx, int64_t batch,
                                    float *u, int64_t ld_u, void *packed_u, void *workspace, size_t ws_bytes, void *stream) {
    return pair_vectors<float>("rtk_pair_vectors_f32", core, a, b, c, S, n_subj, O, n_obj, subject_idx, object_idx, batch, u,
                               ld_u, packed_u, workspace, ws_bytes, stream);
}

extern "C" int rtk_pair_vectors_bf16(const void *core, int a, int b, int c, const void *S, int64_t n_subj, const void *O,
                                     int64_t n_obj, const int64_t *subject_idx, const int64_t *object_idx, int64_t batch,
                                     float *u, int64_t ld_u, void *packed_u, void *workspace, size_t ws_bytes, void *stream) {
    return pair_vectors<rtk_bf16>("rtk_pair_vectors_bf16", (const rtk_bf16 *)core, a, b, c, (const rtk_bf16 *)S, n_subj,
                                  (const rtk_bf16 *)O, n_obj, subject_idx, object_idx, batch, u, ld_u, packed_u, workspace,
                                  ws_bytes, stream);
}
