// Candidate scoring: z[d, k] = v[d] . O[cand[d, k]] for a list of K entities per query (or one list shared by all),
// and its backward (dv by a per-query gather-reduce, dO through a device-built inverted index).  The 1-vs-N kernels
// score every entity; these read only the K rows a query asks for.
//
// Element layout (forward and dv): lane l of a wave holds the elements j = i * CW + l * VW + q of a row
// (chunk i < NCH, q < VW), VW = 16 bytes of the operand type (4 fp32 / 8 bf16), CW = 64 * VW.  A lane sums its
// elements in (i, q) order with fmaf, then the wave adds its 64 lane sums by an xor butterfly.  The layout and so
// the summation order depend on c alone; every candidate is reduced by a whole wave on its own.
#include "rtk_common.h"

namespace {

constexpr int CAND_WAVES = 4;       // waves per workgroup
constexpr int CAND_TILE = 1024;     // entries per wave-tile of the inverted-index sort (64 lanes x 16)
constexpr int CAND_WIN = 256;       // most sorted entries per wave of the dO pass (chunk of a long destination list)

// Entries per wave of the dO pass: M / 4096 (a quarter of a wave's share at 16 waves per CU), 16 to CAND_WIN.  A wave
// walks its window in a chain of dependent loads, so small problems need short windows to fill the chip.
static inline int64_t cand_window(int64_t M) {
    const int64_t w = rtk_cdiv(rtk_cdiv(M, 4096), 16) * 16;
    return w < 16 ? 16 : (w > CAND_WIN ? CAND_WIN : w);
}
constexpr int CAND_MAXC = 1024;

template <typename T> struct Lay {
    static constexpr int VW = sizeof(T) == 4 ? 4 : 8;
    static constexpr int CW = 64 * VW;
};

__device__ __forceinline__ float sum_wave(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);      // commutative pairs: every lane ends with the same bits
    return x;
}

// (through a scalar: a bit_cast straight from the vector element returned element 0 for every q)
__device__ __forceinline__ float bits_elem(const u32x4 &w, int q, float) {
    const unsigned x = w[q];
    return __builtin_bit_cast(float, x);
}
__device__ __forceinline__ float bits_elem(const u32x4 &w, int q, rtk_bf16) {
    const unsigned x = w[q >> 1];
    return __builtin_bit_cast(float, (q & 1) ? (x & 0xffff0000u) : (x << 16));
}

// 16 bytes of row `row` at element j0 (VW elements), zero past c.  VEC: the row is 16-B aligned and c % VW == 0.
template <typename T, bool VEC>
__device__ __forceinline__ u32x4 load_piece(const T *__restrict__ row, int j0, int c) {
    if constexpr (VEC) {
        if (j0 < c) return *reinterpret_cast<const u32x4 *>(row + j0);
        return u32x4{0u, 0u, 0u, 0u};
    }
    u32x4 w{0u, 0u, 0u, 0u};
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = j0 + q < c ? __builtin_bit_cast(unsigned, (float)row[j0 + q]) : 0u;
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned h = j0 + q < c ? (unsigned)row[j0 + q] : 0u;
            w[q >> 1] |= (q & 1) ? (h << 16) : h;
        }
    }
    return w;
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
            for (int i = 0; i < NCH; ++i) o[u][i] = load_piece<T, VEC>(row, i * CW + lane * VW, c);
        }
        float mine = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i)
#pragma unroll
                for (int q = 0; q < VW; ++q) acc = fmaf(vr[i][q], bits_elem(o[u][i], q, T{}), acc);
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
            for (int i = 0; i < NCH; ++i) o[u][i] = load_piece<T, VEC>(row, i * CW + lane * VW, c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (use[u]) {
#pragma unroll
                for (int i = 0; i < NCH; ++i)
#pragma unroll
                    for (int q = 0; q < VW; ++q) acc[i][q] = fmaf(g[u], bits_elem(o[u][i], q, T{}), acc[i][q]);
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

// ---- inverted index: entries i = d K + k sorted by entity (stable: increasing i within an entity) ----------------
// Invalid candidates get the key n_ent and sort last.
__global__ __launch_bounds__(256) void cand_keys_kernel(const int64_t *__restrict__ cand, int64_t ld_cand, int64_t K,
                                                       int64_t n_ent, int64_t M, int32_t *__restrict__ keys,
                                                       int32_t *__restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int64_t d = i / K, k = i - d * K;
        const int64_t e = cand[d * ld_cand + k];
        keys[i] = (int32_t)(e >= 0 && e < n_ent ? e : n_ent);
        vals[i] = (int32_t)i;
    }
}

// One radix pass (8 bits at `shift`): wave-tile digit counts, stored digit-major [digit][tile].
__global__ __launch_bounds__(256) void cand_hist_kernel(const int32_t *__restrict__ keys, int64_t M, int shift,
                                                       int64_t ntiles, int32_t *__restrict__ hist) {
    __shared__ int h[CAND_WAVES][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * CAND_WAVES + wv;
    for (int i = lane; i < 256; i += 64) h[wv][i] = 0;
    __syncthreads();
    if (tile < ntiles)
        for (int it = 0; it < CAND_TILE / 64; ++it) {
            const int64_t idx = tile * CAND_TILE + it * 64 + lane;
            if (idx < M) atomicAdd(&h[wv][(keys[idx] >> shift) & 255], 1);
        }
    __syncthreads();
    if (tile < ntiles)
        for (int i = lane; i < 256; i += 64) hist[(int64_t)i * ntiles + tile] = h[wv][i];
}

// Scatter of one radix pass: a wave walks its tile in order, 64 entries at a time; lanes with equal digits are
// matched by 8 ballots and placed in lane order behind the digit's running cursor -> stable.
__global__ __launch_bounds__(256) void cand_scatter_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ vals,
                                                          int64_t M, int shift, int64_t ntiles,
                                                          const int32_t *__restrict__ offs, int32_t *__restrict__ keys_out,
                                                          int32_t *__restrict__ vals_out) {
    __shared__ int cur[CAND_WAVES][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * CAND_WAVES + wv;
    if (tile >= ntiles) return;
    for (int i = lane; i < 256; i += 64) cur[wv][i] = offs[(int64_t)i * ntiles + tile];
    __builtin_amdgcn_wave_barrier();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int it = 0; it < CAND_TILE / 64; ++it) {
        const int64_t idx = tile * CAND_TILE + it * 64 + lane;
        const bool valid = idx < M;
        const int32_t key = valid ? keys[idx] : 0;
        const int32_t val = valid ? vals[idx] : 0;
        const int dg = (key >> shift) & 255;
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bb = __ballot((dg >> b) & 1);
            m &= ((dg >> b) & 1) ? bb : ~bb;
        }
        const int rank = __popcll(m & lt);
        const int base = valid ? cur[wv][dg] : 0;
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) cur[wv][dg] = base + __popcll(m);
        if (valid && base + rank < M) {                   // (always true for consistent counts)
            keys_out[base + rank] = key;
            vals_out[base + rank] = val;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Exclusive scan of n int32 in blocks of 4096 (256 threads x 16): block totals, scan of the totals, final pass.
constexpr int SCAN_IT = 16, SCAN_BLK = 256 * SCAN_IT;

__device__ int block_excl_scan(int x, int *lds, int *total) {     // 256 threads; returns the exclusive prefix of x
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        before += i < wv ? lds[i] : 0;
        tot += lds[i];
    }
    __syncthreads();
    *total = tot;
    return before + inc - x;
}

__global__ __launch_bounds__(256) void scan_totals_kernel(const int32_t *__restrict__ a, int64_t n, int32_t *__restrict__ bs) {
    __shared__ int lds[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_IT;
    int s = 0;
    for (int q = 0; q < SCAN_IT; ++q) s += base + q < n ? a[base + q] : 0;
    int tot;
    block_excl_scan(s, lds, &tot);
    if (threadIdx.x == 0) bs[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void scan_blocks_kernel(int32_t *__restrict__ bs, int64_t nb) {
    __shared__ int lds[4];
    int carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t i = b0 + threadIdx.x;
        const int x = i < nb ? bs[i] : 0;
        int tot;
        const int ex = block_excl_scan(x, lds, &tot);
        if (i < nb) bs[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(256) void scan_final_kernel(const int32_t *__restrict__ a, int64_t n,
                                                        const int32_t *__restrict__ bs, int32_t *__restrict__ out) {
    __shared__ int lds[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_IT;
    int x[SCAN_IT];
    int s = 0;
#pragma unroll
    for (int q = 0; q < SCAN_IT; ++q) {
        x[q] = base + q < n ? a[base + q] : 0;
        s += x[q];
    }
    int tot;
    int run = bs[blockIdx.x] + block_excl_scan(s, lds, &tot);
#pragma unroll
    for (int q = 0; q < SCAN_IT; ++q) {
        if (base + q < n) out[base + q] = run;
        run += x[q];
    }
}

// dO: wave w sums the sorted entries [w win, (w + 1) win) run by run (a run = one entity), in sorted order.  A run
// wholly inside the window is written to gO; a run that started in an earlier window leaves its partial sum in
// slot 0 of the window, one that starts here and goes on in slot 1.  The rows of v use the fp32 layout.
template <int NCH, bool VEC>
__device__ __forceinline__ void store_row(float *__restrict__ dst, const float (&acc)[NCH][4], int c, int lane) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int j0 = i * 256 + lane * 4;
        if (VEC) {
            if (j0 < c) *reinterpret_cast<f32x4 *>(dst + j0) = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j0 + q < c) dst[j0 + q] = acc[i][q];
        }
    }
}

template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void cand_go_kernel(const int32_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                     int64_t M, int64_t n_ent, const float *__restrict__ dz,
                                                     int64_t ld_dz, int64_t K, const float *__restrict__ v, int c,
                                                     float *__restrict__ gO, float *__restrict__ P, int64_t win,
                                                     const int32_t *__restrict__ owner) {
    constexpr int U = NCH <= 2 ? 8 : 4;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * CAND_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p0 = w * win;
    if (p0 >= M) return;
    const int64_t p1 = p0 + win < M ? p0 + win : M;
    const int32_t key_prev = p0 > 0 ? skey[p0 - 1] : -1;
    const int32_t key_next = p1 < M ? skey[p1] : -1;
    float acc[NCH][4];
    auto zero = [&]() {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
    };
    zero();
    int32_t cur = skey[p0];
    bool first = true;
    auto flush = [&](bool continues) {
        if (cur < 0 || cur >= n_ent) return;                         // invalid candidates (sorted last) add nothing
        const bool before = first && key_prev == cur;
        float *dst = before ? P + (w * 2 + 0) * CAND_MAXC : continues ? P + (w * 2 + 1) * CAND_MAXC
                                                                      : gO + (int64_t)cur * c;
        if (before || continues) store_row<NCH, true>(dst, acc, CAND_MAXC, lane);
        else store_row<NCH, VEC>(dst, acc, c, lane);
    };
    for (int64_t pb = p0; pb < p1; pb += U) {
        int32_t kk[U];
        float g[U];
        int64_t dd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = pb + u < p1;
            kk[u] = in ? skey[pb + u] : -1;
            int64_t i = in ? sval[pb + u] : 0;
            i = i < 0 ? 0 : (i >= M ? M - 1 : i);
            dd[u] = i / K;
            g[u] = in && kk[u] < n_ent ? dz[dd[u] * ld_dz + (i - dd[u] * K)] : 0.f;
        }
        u32x4 x[U][NCH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t vr = owner ? (int64_t)owner[dd[u]] : dd[u];      // flat list (K = 1): entry -> its query
#pragma unroll
            for (int i = 0; i < NCH; ++i) x[u][i] = load_piece<float, VEC>(v + vr * c, i * 256 + lane * 4, c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kk[u] < 0) break;
            if (kk[u] != cur) {
                flush(false);
                zero();
                cur = kk[u];
                first = false;
            }
#pragma unroll
            for (int i = 0; i < NCH; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(g[u], bits_elem(x[u][i], q, 0.f), acc[i][q]);
        }
    }
    flush(key_next == cur);
}

// The runs that cross windows: the window where a run starts adds its slot-1 partial and the slot-0 partials of
// the following windows, in window order, and writes the destination row.
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void cand_go_combine_kernel(const int32_t *__restrict__ skey, int64_t M, int64_t n_ent,
                                                             int c, float *__restrict__ gO, const float *__restrict__ P,
                                                             int64_t win) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * CAND_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p0 = w * win;
    if (p0 >= M) return;
    const int64_t p1 = p0 + win < M ? p0 + win : M;
    if (p1 >= M) return;
    const int32_t e = skey[p1 - 1];
    if (e < 0 || e >= n_ent || skey[p1] != e) return;                            // the window's last run ends inside it
    if (skey[p0] == e && p0 > 0 && skey[p0 - 1] == e) return;            // ... or started in an earlier window
    float acc[NCH][4];
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = P[(w * 2 + 1) * CAND_MAXC + i * 256 + lane * 4 + q];
    for (int64_t w2 = w + 1;; ++w2) {
        const float *src = P + (w2 * 2 + 0) * CAND_MAXC;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] += src[i * 256 + lane * 4 + q];
        const int64_t q1 = (w2 + 1) * win;
        if (q1 >= M || skey[q1] != e) break;
    }
    store_row<NCH, VEC>(gO + (int64_t)e * c, acc, c, lane);
}

struct CandWs {
    int32_t *keys[2], *vals[2], *hist, *offs, *bs;
    float *P;
    int64_t M, ntiles, nh, nb, win, nwin;
    size_t total;
};
CandWs carve_cand(void *base, int64_t batch, int64_t k) {
    CandWs w;
    unsigned char *p = (unsigned char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char *q = p ? p + off : nullptr;
        off += rtk_align_up(bytes, 256);
        return q;
    };
    w.M = batch * k;
    w.ntiles = rtk_cdiv(w.M, CAND_TILE);
    w.nh = 256 * w.ntiles;
    w.nb = rtk_cdiv(w.nh, SCAN_BLK);
    w.win = cand_window(w.M);
    w.nwin = rtk_cdiv(w.M, w.win);
    for (int i = 0; i < 2; ++i) {
        w.keys[i] = (int32_t *)take((size_t)w.M * 4);
        w.vals[i] = (int32_t *)take((size_t)w.M * 4);
    }
    w.hist = (int32_t *)take((size_t)w.nh * 4);
    w.offs = (int32_t *)take((size_t)w.nh * 4);
    w.bs = (int32_t *)take((size_t)(w.nb + 1) * 4);
    w.P = (float *)take((size_t)w.nwin * 2 * CAND_MAXC * 4);
    w.total = off;
    return w;
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
    auto go = [&](auto nc, auto sg, auto vc) {
        RTK_LAUNCH_SCORE((cand_fwd_kernel<T, decltype(nc)::value, decltype(sg)::value, decltype(vc)::value>),
                         dim3((unsigned)blocks), dim3(256), 0, st, v, batch, c, O, n_ent, cand, ld_cand, k, span, nspan,
                         out, ld_out, err);
        return RTK_OK;
    };
    auto by_vec = [&](auto nc, auto sg) {
        return vec ? go(nc, sg, std::true_type{}) : go(nc, sg, std::false_type{});
    };
    auto by_sig = [&](auto nc) {
        return sig == 0 ? by_vec(nc, std::integral_constant<int, 0>{})
             : sig == 1 ? by_vec(nc, std::integral_constant<int, 1>{}) : by_vec(nc, std::integral_constant<int, 2>{});
    };
    if (nch == 1) by_sig(std::integral_constant<int, 1>{});
    else if (nch == 2) by_sig(std::integral_constant<int, 2>{});
    else if constexpr (sizeof(T) == 4) {
        if (nch == 3) by_sig(std::integral_constant<int, 3>{});
        else by_sig(std::integral_constant<int, 4>{});
    }
    return rtk_check_launch(fn);
}

// Flat front end of the ordered scatter (rtk_bce_stream.hip: the positives of a ragged CSR): M entries (entity ent[i],
// query owner[i], logit gradient dz[i]); an entity outside [0, n_ent) adds nothing.  gO is zeroed, then written.  The
// bits of gO depend on the entries alone, not on how many surplus slots M leaves behind them.
__global__ __launch_bounds__(256) void flat_keys_kernel(const int32_t *__restrict__ ent, int64_t n_ent, int64_t M,
                                                       int32_t *__restrict__ keys, int32_t *__restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int32_t e = ent[i];
        keys[i] = e >= 0 && e < n_ent ? e : (int32_t)n_ent;
        vals[i] = (int32_t)i;
    }
}

// The keys / vals of ws.keys[0], ws.vals[0] sorted by entity (stable), then the ordered sums into gO (zeroed by the caller).
// `owner` (flat lists, k = 1): entry i belongs to query owner[i]; null: to query i / k.
int sorted_scatter(const char *fn, const CandWs &ws, int64_t n_ent, const float *dz, int64_t ld_dz, int64_t k,
                   const int32_t *owner, const float *v, int c, float *gO, hipStream_t st) {
    const int64_t M = ws.M;
    int bits = 1;
    while ((n_ent >> bits) != 0) ++bits;             // keys are <= n_ent
    const unsigned tblocks = (unsigned)rtk_cdiv(ws.ntiles, CAND_WAVES);
    int src = 0;
    for (int shift = 0; shift < bits; shift += 8, src ^= 1) {
        hipLaunchKernelGGL(cand_hist_kernel, dim3(tblocks), dim3(256), 0, st, ws.keys[src], M, shift, ws.ntiles, ws.hist);
        hipLaunchKernelGGL(scan_totals_kernel, dim3((unsigned)ws.nb), dim3(256), 0, st, ws.hist, ws.nh, ws.bs);
        hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, st, ws.bs, ws.nb);
        hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)ws.nb), dim3(256), 0, st, ws.hist, ws.nh, ws.bs, ws.offs);
        hipLaunchKernelGGL(cand_scatter_kernel, dim3(tblocks), dim3(256), 0, st, ws.keys[src], ws.vals[src], M, shift,
                           ws.ntiles, ws.offs, ws.keys[src ^ 1], ws.vals[src ^ 1]);
    }
    const bool vec = c % 4 == 0 && ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(gO)) & 15) == 0;
    const unsigned wblocks = (unsigned)rtk_cdiv(ws.nwin, CAND_WAVES);
    auto go = [&](auto nc, auto vc) {
        constexpr int NC = decltype(nc)::value;
        constexpr bool VC = decltype(vc)::value;
        RTK_LAUNCH_SCORE((cand_go_kernel<NC, VC>), dim3(wblocks), dim3(256), 0, st, ws.keys[src], ws.vals[src], M, n_ent,
                         dz, ld_dz, k, v, c, gO, ws.P, ws.win, owner);
        hipLaunchKernelGGL((cand_go_combine_kernel<NC, VC>), dim3(wblocks), dim3(256), 0, st, ws.keys[src], M, n_ent, c, gO,
                           ws.P, ws.win);
    };
    auto by_vec = [&](auto nc) { vec ? go(nc, std::true_type{}) : go(nc, std::false_type{}); };
    const int nch = (c + 255) / 256;
    if (nch == 1) by_vec(std::integral_constant<int, 1>{});
    else if (nch == 2) by_vec(std::integral_constant<int, 2>{});
    else if (nch == 3) by_vec(std::integral_constant<int, 3>{});
    else by_vec(std::integral_constant<int, 4>{});
    return rtk_check_launch(fn);
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
            const hipError_t e = hipMemsetAsync(dv, 0, (size_t)batch * c * 4, st);
            if (e != hipSuccess) {
                rtk_set_error("%s: memset: %s", fn, hipGetErrorString(e));
                return RTK_ERR_LAUNCH;
            }
        } else {
            constexpr int VW = Lay<T>::VW, CW = Lay<T>::CW;
            const bool vec = c % VW == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0;
            const int nch = (c + CW - 1) / CW;
            auto go = [&](auto nc, auto vc) {
                RTK_LAUNCH_SCORE((cand_dv_kernel<T, decltype(nc)::value, decltype(vc)::value>), dim3((unsigned)batch),
                                 dim3(256), 0, st, dz, ld_dz, c, O, n_ent, cand, ld_cand, k, dv);
            };
            auto by_vec = [&](auto nc) { vec ? go(nc, std::true_type{}) : go(nc, std::false_type{}); };
            if (nch == 1) by_vec(std::integral_constant<int, 1>{});
            else if (nch == 2) by_vec(std::integral_constant<int, 2>{});
            else if constexpr (sizeof(T) == 4) {
                if (nch == 3) by_vec(std::integral_constant<int, 3>{});
                else by_vec(std::integral_constant<int, 4>{});
            }
            rc = rtk_check_launch(fn);
            if (rc != RTK_OK) return rc;
        }
    }
    if (!gO) return RTK_OK;
    hipError_t e = hipMemsetAsync(gO, 0, (size_t)n_ent * c * 4, st);
    if (e != hipSuccess) {
        rtk_set_error("%s: memset: %s", fn, hipGetErrorString(e));
        return RTK_ERR_LAUNCH;
    }
    const CandWs ws = carve_cand(workspace, batch, k);
    const int64_t M = ws.M;
    if (M == 0) return RTK_OK;
    const unsigned gblocks = (unsigned)(rtk_cdiv(M, 256) < 4096 ? rtk_cdiv(M, 256) : 4096);
    hipLaunchKernelGGL(cand_keys_kernel, dim3(gblocks), dim3(256), 0, st, cand, ld_cand, k, n_ent, M, ws.keys[0], ws.vals[0]);
    return sorted_scatter(fn, ws, n_ent, dz, ld_dz, k, nullptr, v, c, gO, st);
}

}  // namespace

size_t rtk_cand_flat_workspace_bytes(int64_t m) { return m <= 0 ? 0 : carve_cand(nullptr, m, 1).total; }

int rtk_cand_flat_scatter(const char *fn, const int32_t *ent, const int32_t *owner, const float *dz, int64_t m,
                          int64_t n_ent, const float *v, int c, float *gO, void *workspace, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(gO, 0, (size_t)n_ent * c * 4, st);
    if (e != hipSuccess) {
        rtk_set_error("%s: memset: %s", fn, hipGetErrorString(e));
        return RTK_ERR_LAUNCH;
    }
    if (m <= 0) return RTK_OK;
    CandWs ws = carve_cand(workspace, m, 1);
    // m is the caller's BOUND on the entries (the surplus slots sort last and add nothing): the sums must not depend on
    // it, so the flat lists are always cut into windows of CAND_WIN, which P -- carved for cand_window(m) <= CAND_WIN -- holds
    ws.win = CAND_WIN;
    ws.nwin = rtk_cdiv(ws.M, ws.win);
    const unsigned gblocks = (unsigned)(rtk_cdiv(m, 256) < 4096 ? rtk_cdiv(m, 256) : 4096);
    hipLaunchKernelGGL(flat_keys_kernel, dim3(gblocks), dim3(256), 0, st, ent, n_ent, m, ws.keys[0], ws.vals[0]);
    return sorted_scatter(fn, ws, n_ent, dz, 1, 1, owner, v, c, gO, st);
}

extern "C" size_t rtk_score_candidates_bwd_workspace_bytes(int64_t batch, int64_t k, int64_t n_ent) {
    if (batch <= 0 || k <= 0 || n_ent <= 0 || batch >= (1ll << 31) || k >= (1ll << 31) || batch * k >= (1ll << 31)) return 0;
    return carve_cand(nullptr, batch, k).total;
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
