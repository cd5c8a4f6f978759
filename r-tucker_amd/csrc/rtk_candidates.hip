// Candidate scoring: z[d, k] = v[d] . O[cand[d, k]] for a list of K entities per query (or one list shared by all),
// and its backward (dv by a per-query gather-reduce, dO through the ordered scatter of rtk_scatter.h).  The 1-vs-N kernels
// score every entity; these read only the K rows a query asks for.
//
// Element layout (forward and dv): lane l of a wave holds the elements j = i * CW + l * VW + q of a row
// (chunk i < NCH, q < VW), VW = 16 bytes of the operand type (4 fp32 / 8 bf16), CW = 64 * VW.  A lane sums its
// elements in (i, q) order with fmaf, then the wave adds its 64 lane sums by an xor butterfly.  The layout and so
// the summation order depend on c alone; every candidate is reduced by a whole wave on its own.
#include "rtk_common.h"
#include "rtk_scatter.h"

namespace {

constexpr int CAND_WAVES = 4;       // waves per workgroup
constexpr int CAND_MAXC = RTK_SCATTER_MAXC;

template <typename T> struct Lay {
    static constexpr int VW = sizeof(T) == 4 ? 4 : 8;
    static constexpr int CW = 64 * VW;
};

__device__ __forceinline__ float sum_wave(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);      // commutative pairs: every lane ends with the same bits
    return x;
}

template <int SIG> __device__ __forceinline__ float logistic(float z) {
    if (SIG == 2) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
    if (SIG == 1) return rtk_sigmoid(z);
    return z;
}

// Forward.  Wave w scores candidates [k0, k0 + span) of query d = w / nspan; U rows in flight per wave.
template <typename T, int NCH, int SIG, bool VEC>
__global__ __launch_bounds__(256) void cand_fwd_kernel(const float *__restrict__ v, int64_t batch, int c,
                                                      const T *__restrict__ O, int64_t n_ent,
                                                      const int64_t *__restrict__ cand, int64_t ld_cand, int64_t K,
                                                      int64_t span, int64_t nspan, float *__restrict__ out,
                                                      int64_t ld_out, uint32_t *__restrict__ err) {
    constexpr int VW = Lay<T>::VW, CW = Lay<T>::CW;
    constexpr int U = NCH <= 2 ? 8 : 4;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * CAND_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= batch * nspan) return;
    const int64_t d = w / nspan;
    const int64_t k0 = (w - d * nspan) * span;
    const int64_t k1 = k0 + span < K ? k0 + span : K;
    float vr[NCH][VW];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int q = 0; q < VW; ++q) {
            const int j = i * CW + lane * VW + q;
            const float x = j < c ? v[d * c + j] : 0.f;
            vr[i][q] = sizeof(T) == 4 ? x : rtk_to_f32(rtk_f32_to_bf16(x));     // bf16 operands: v rounded to bf16
        }
    const int64_t *cd = cand + d * ld_cand;
    float *od = out + d * ld_out;
    bool bad = false;
    for (int64_t kb = k0; kb < k1; kb += U) {
        int64_t e[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = kb + u < k1;
            const int64_t id = in ? cd[kb + u] : 0;
            ok[u] = id >= 0 && id < n_ent;
            bad |= in && !ok[u];
            e[u] = id < 0 ? 0 : (id >= n_ent ? n_ent - 1 : id);        // clamped for the load
        }
        u32x4 o[U][NCH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T *row = O + e[u] * (int64_t)c;
#pragma unroll
            for (int i = 0; i < NCH; ++i) o[u][i] = rtk_load_piece<T, VEC>(row, i * CW + lane * VW, c);
        }
        float mine = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i)
#pragma unroll
                for (int q = 0; q < VW; ++q) acc = fmaf(vr[i][q], rtk_bits_elem(o[u][i], q, T{}), acc);
            acc = sum_wave(acc);
            if (lane == u) mine = ok[u] ? logistic<SIG>(acc) : __builtin_nanf("");
        }
        if (lane < U && kb + lane < k1) od[kb + lane] = mine;
    }
    if (bad && lane == 0) atomicOr(err, 2u);
}

// dv[d, :] = sum_k dZ[d, k] O[cand[d, k], :].  One workgroup per query; wave wv adds the k of its quarter of the
// list in increasing k, and wave 0 adds the four partial sums in wave order.  Out-of-range candidates add nothing.
template <typename T, int NCH, bool VEC>
__global__ __launch_bounds__(256) void cand_dv_kernel(const float *__restrict__ dz, int64_t ld_dz, int c,
                                                     const T *__restrict__ O, int64_t n_ent,
                                                     const int64_t *__restrict__ cand, int64_t ld_cand, int64_t K,
                                                     float *__restrict__ dv) {
    constexpr int VW = Lay<T>::VW, CW = Lay<T>::CW;
    constexpr int U = NCH <= 2 ? 8 : 4;
    __shared__ float part[CAND_WAVES - 1][NCH * VW][64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t d = blockIdx.x;
    const int64_t quarter = (K + CAND_WAVES - 1) / CAND_WAVES;
    const int64_t k0 = wv * quarter, k1 = k0 + quarter < K ? k0 + quarter : K;
    const int64_t *cd = cand + d * ld_cand;
    const float *zd = dz + d * ld_dz;
    float acc[NCH][VW];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int q = 0; q < VW; ++q) acc[i][q] = 0.f;
    for (int64_t kb = k0; kb < k1; kb += U) {
        int64_t e[U];
        float g[U];
        bool use[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = kb + u < k1;
            const int64_t id = in ? cd[kb + u] : 0;
            use[u] = in && id >= 0 && id < n_ent;
            e[u] = use[u] ? id : 0;
            g[u] = use[u] ? zd[kb + u] : 0.f;
        }
        u32x4 o[U][NCH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T *row = O + e[u] * (int64_t)c;
#pragma unroll
            for (int i = 0; i < NCH; ++i) o[u][i] = rtk_load_piece<T, VEC>(row, i * CW + lane * VW, c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (use[u]) {
#pragma unroll
                for (int i = 0; i < NCH; ++i)
#pragma unroll
                    for (int q = 0; q < VW; ++q) acc[i][q] = fmaf(g[u], rtk_bits_elem(o[u][i], q, T{}), acc[i][q]);
            }
    }
    if (wv > 0) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int q = 0; q < VW; ++q) part[wv - 1][i * VW + q][lane] = acc[i][q];
    }
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int q = 0; q < VW; ++q) {
            float s = acc[i][q];
#pragma unroll
            for (int p = 0; p < CAND_WAVES - 1; ++p) s += part[p][i * VW + q][lane];
            const int j = i * CW + lane * VW + q;
            if (j < c) dv[d * c + j] = s;
        }
}

int check_args(const char *fn, const void *v, int64_t batch, int c, const void *O, int64_t n_ent, const int64_t *cand,
               int64_t ld_cand, int64_t k) {
    RTK_REQUIRE(v && O && cand, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(c >= 1, RTK_ERR_BAD_ARG, "%s: object rank c = %d must be >= 1", fn, c);
    RTK_REQUIRE(c <= CAND_MAXC, RTK_ERR_UNSUPPORTED, "%s: object rank c = %d above %d", fn, c, CAND_MAXC);
    RTK_REQUIRE(batch >= 0 && k >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld and K = %lld must be >= 0", fn, (long long)batch,
                (long long)k);
    RTK_REQUIRE(n_ent >= 1 && n_ent < (1ll << 31) - 1, RTK_ERR_BAD_ARG, "%s: n_ent = %lld outside [1, 2^31 - 1)", fn,
                (long long)n_ent);
    RTK_REQUIRE(ld_cand == 0 || ld_cand >= k, RTK_ERR_BAD_ARG, "%s: ld_cand = %lld must be 0 (one shared list) or >= K = %lld",
                fn, (long long)ld_cand, (long long)k);
    RTK_REQUIRE(batch < (1ll << 31) && k < (1ll << 31) && batch * k < (1ll << 31), RTK_ERR_UNSUPPORTED,
                "%s: batch x K = %lld x %lld above 2^31 entries", fn, (long long)batch, (long long)k);
    return RTK_OK;
}

template <typename T>
int score_candidates(const char *fn, const float *v, int64_t batch, int c, const T *O, int64_t n_ent,
                     const int64_t *cand, int64_t ld_cand, int64_t k, float *out, int64_t ld_out, unsigned flags,
                     void *workspace, size_t workspace_bytes, void *stream) {
    int rc = check_args(fn, v, batch, c, O, n_ent, cand, ld_cand, k);
    if (rc != RTK_OK) return rc;
    RTK_REQUIRE(out, RTK_ERR_BAD_ARG, "%s: null output", fn);
    RTK_REQUIRE(ld_out >= k, RTK_ERR_BAD_ARG, "%s: ld_out = %lld < K = %lld", fn, (long long)ld_out, (long long)k);
    RTK_REQUIRE((flags & ~(RTK_SCORE_SIGMOID | RTK_SCORE_SIGMOID_FAST)) == 0, RTK_ERR_BAD_ARG, "%s: unknown flags 0x%x",
                fn, flags);
    RTK_REQUIRE(workspace && workspace_bytes >= 256, RTK_ERR_BAD_ARG, "%s: workspace of %zu bytes given, 256 needed", fn,
                workspace_bytes);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_BAD_ARG, "%s: workspace must be 256-byte aligned",
                fn);
    if (batch == 0 || k == 0) return RTK_OK;
    constexpr int VW = Lay<T>::VW, CW = Lay<T>::CW;
    const bool vec = c % VW == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0;
    const int nch = (c + CW - 1) / CW;
    // about 16 waves per CU x 4 rounds over the chip; a span is a multiple of 8 rows (the rows in flight)
    int64_t span = rtk_cdiv(batch * k, 16384);
    span = rtk_cdiv(span, 8) * 8;
    if (span > k) span = k;
    const int64_t nspan = rtk_cdiv(k, span);
    const int64_t blocks = rtk_cdiv(batch * nspan, CAND_WAVES);
    const int sig = !(flags & RTK_SCORE_SIGMOID) ? 0 : (flags & RTK_SCORE_SIGMOID_FAST) ? 2 : 1;
    hipStream_t st = (hipStream_t)stream;
    uint32_t *err = (uint32_t *)workspace;
    return rtk_dispatch_chunks<sizeof(T) == 4 ? 4 : 2>(fn, nch, vec, [&](auto nc, auto vc) {
        auto go = [&](auto sg) {
            RTK_LAUNCH_SCORE((cand_fwd_kernel<T, decltype(nc)::value, decltype(sg)::value, decltype(vc)::value>),
                             dim3((unsigned)blocks), dim3(256), 0, st, v, batch, c, O, n_ent, cand, ld_cand, k, span, nspan,
                             out, ld_out, err);
        };
        sig == 0 ? go(std::integral_constant<int, 0>{}) : sig == 1 ? go(std::integral_constant<int, 1>{})
                                                                    : go(std::integral_constant<int, 2>{});
    });
}

template <typename T>
int score_candidates_bwd(const char *fn, const float *dz, int64_t ld_dz, const float *v, int64_t batch, int c, const T *O,
                         int64_t n_ent, const int64_t *cand, int64_t ld_cand, int64_t k, float *dv, float *gO,
                         void *workspace, size_t workspace_bytes, void *stream) {
    int rc = check_args(fn, v, batch, c, O, n_ent, cand, ld_cand, k);
    if (rc != RTK_OK) return rc;
    RTK_REQUIRE(dz, RTK_ERR_BAD_ARG, "%s: null dZ", fn);
    RTK_REQUIRE(ld_dz >= k, RTK_ERR_BAD_ARG, "%s: ld_dz = %lld < K = %lld", fn, (long long)ld_dz, (long long)k);
    if (gO) {
        const size_t need = rtk_score_candidates_bwd_workspace_bytes(batch, k, n_ent);
        RTK_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), RTK_ERR_BAD_ARG,
                    "%s: workspace of %zu bytes given, %zu needed", fn, workspace_bytes, need);
        RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_BAD_ARG,
                    "%s: workspace must be 256-byte aligned", fn);
    }
    hipStream_t st = (hipStream_t)stream;
    if (dv && batch > 0) {
        if (k == 0) {
            rc = rtk_zero_async(fn, dv, (size_t)batch * c * 4, st);
        } else {
            constexpr int VW = Lay<T>::VW, CW = Lay<T>::CW;
            const bool vec = c % VW == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0;
            rc = rtk_dispatch_chunks<sizeof(T) == 4 ? 4 : 2>(fn, (c + CW - 1) / CW, vec, [&](auto nc, auto vc) {
                RTK_LAUNCH_SCORE((cand_dv_kernel<T, decltype(nc)::value, decltype(vc)::value>), dim3((unsigned)batch),
                                 dim3(256), 0, st, dz, ld_dz, c, O, n_ent, cand, ld_cand, k, dv);
            });
        }
        if (rc != RTK_OK) return rc;
    }
    if (!gO) return RTK_OK;
    return rtk_scatter_candidates(fn, cand, ld_cand, batch, k, n_ent, dz, ld_dz, v, c, gO, workspace, st);
}

}  // namespace

extern "C" size_t rtk_score_candidates_bwd_workspace_bytes(int64_t batch, int64_t k, int64_t n_ent) {
    if (batch <= 0 || k <= 0 || n_ent <= 0 || batch >= (1ll << 31) || k >= (1ll << 31) || batch * k >= (1ll << 31)) return 0;
    return rtk_scatter_bytes(batch * k);
}

extern "C" int rtk_score_candidates_f32(const float *v, int64_t batch, int c, const float *O, int64_t n_ent,
                                        const int64_t *cand, int64_t ld_cand, int64_t k, float *out, int64_t ld_out,
                                        unsigned flags, void *workspace, size_t workspace_bytes, void *stream) {
    return score_candidates<float>("rtk_score_candidates_f32", v, batch, c, O, n_ent, cand, ld_cand, k, out, ld_out, flags,
                                   workspace, workspace_bytes, stream);
}

extern "C" int rtk_score_candidates_bf16(const float *v, int64_t batch, int c, const void *O, int64_t n_ent,
                                         const int64_t *cand, int64_t ld_cand, int64_t k, float *out, int64_t ld_out,
                                         unsigned flags, void *workspace, size_t workspace_bytes, void *stream) {
    return score_candidates<rtk_bf16>("rtk_score_candidates_bf16", v, batch, c, (const rtk_bf16 *)O, n_ent, cand, ld_cand, k,
                                      out, ld_out, flags, workspace, workspace_bytes, stream);
}

extern "C" int rtk_score_candidates_bwd_f32(const float *dz, int64_t ld_dz, const float *v, int64_t batch, int c,
                                            const float *O, int64_t n_ent, const int64_t *cand, int64_t ld_cand, int64_t k,
                                            float *dv, float *gO, void *workspace, size_t workspace_bytes, void *stream) {
    return score_candidates_bwd<float>("rtk_score_candidates_bwd_f32", dz, ld_dz, v, batch, c, O, n_ent, cand, ld_cand, k,
                                       dv, gO, workspace, workspace_bytes, stream);
}

extern "C" int rtk_score_candidates_bwd_bf16(const float *dz, int64_t ld_dz, const float *v, int64_t batch, int c,
                                             const void *O, int64_t n_ent, const int64_t *cand, int64_t ld_cand, int64_t k,
                                             float *dv, float *gO, void *workspace, size_t workspace_bytes, void *stream) {
    return score_candidates_bwd<rtk_bf16>("rtk_score_candidates_bwd_bf16", dz, ld_dz, v, batch, c, (const rtk_bf16 *)O,
                                          n_ent, cand, ld_cand, k, dv, gO, workspace, workspace_bytes, stream);
}
