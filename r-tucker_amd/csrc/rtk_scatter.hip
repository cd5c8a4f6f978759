// The ordered scatter: gO[e, :] = sum of dz[i] v[query of i, :] over the entries i of entity e, in a fixed order (the
// order and the two front ends' windows: rtk_scatter.h).  A stable LSD radix sort of the entries by entity, a windowed
// run sum in sorted order, and a combine pass for the runs that cross windows.
#include "rtk_scatter.h"

namespace {

constexpr int SC_WAVES = 4;         // waves per workgroup
constexpr int SC_TILE = 1024;       // entries per wave-tile of the sort (64 lanes x 16)

// ---- the keys of the two front ends: an entity outside [0, n_ent) gets the key n_ent and sorts last --------------
// candidate matrix: entry i = d K + k
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

// flat lists: entry i
__global__ __launch_bounds__(256) void flat_keys_kernel(const int32_t *__restrict__ ent, int64_t n_ent, int64_t M,
                                                       int32_t *__restrict__ keys, int32_t *__restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int32_t e = ent[i];
        keys[i] = e >= 0 && e < n_ent ? e : (int32_t)n_ent;
        vals[i] = (int32_t)i;
    }
}

// ---- the sort by key (stable: increasing i within an entity) -----------------------------------------------------
// One radix pass (8 bits at `shift`): wave-tile digit counts, stored digit-major [digit][tile].
__global__ __launch_bounds__(256) void sort_hist_kernel(const int32_t *__restrict__ keys, int64_t M, int shift,
                                                       int64_t ntiles, int32_t *__restrict__ hist) {
    __shared__ int h[SC_WAVES][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * SC_WAVES + wv;
    for (int i = lane; i < 256; i += 64) h[wv][i] = 0;
    __syncthreads();
    if (tile < ntiles)
        for (int it = 0; it < SC_TILE / 64; ++it) {
            const int64_t idx = tile * SC_TILE + it * 64 + lane;
            if (idx < M) atomicAdd(&h[wv][(keys[idx] >> shift) & 255], 1);
        }
    __syncthreads();
    if (tile < ntiles)
        for (int i = lane; i < 256; i += 64) hist[(int64_t)i * ntiles + tile] = h[wv][i];
}

// Scatter of one radix pass: a wave walks its tile in order, 64 entries at a time; lanes with equal digits are
// matched by 8 ballots and placed in lane order behind the digit's running cursor -> stable.
__global__ __launch_bounds__(256) void sort_place_kernel(const int32_t *__restrict__ keys, const int32_t *__restrict__ vals,
                                                          int64_t M, int shift, int64_t ntiles,
                                                          const int32_t *__restrict__ offs, int32_t *__restrict__ keys_out,
                                                          int32_t *__restrict__ vals_out) {
    __shared__ int cur[SC_WAVES][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * SC_WAVES + wv;
    if (tile >= ntiles) return;
    for (int i = lane; i < 256; i += 64) cur[wv][i] = offs[(int64_t)i * ntiles + tile];
    __builtin_amdgcn_wave_barrier();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int it = 0; it < SC_TILE / 64; ++it) {
        const int64_t idx = tile * SC_TILE + it * 64 + lane;
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
__global__ __launch_bounds__(256) void run_sum_kernel(const int32_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                     int64_t M, int64_t n_ent, const float *__restrict__ dz,
                                                     int64_t ld_dz, int64_t K, const float *__restrict__ v, int64_t ld_v,
                                                     int c, float *__restrict__ gO, float *__restrict__ P, int64_t win,
                                                     const int32_t *__restrict__ owner) {
    constexpr int U = NCH <= 2 ? 8 : 4;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * SC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
        float *dst = before ? P + (w * 2 + 0) * RTK_SCATTER_MAXC : continues ? P + (w * 2 + 1) * RTK_SCATTER_MAXC
                                                                      : gO + (int64_t)cur * c;
        if (before || continues) store_row<NCH, true>(dst, acc, RTK_SCATTER_MAXC, lane);
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
            for (int i = 0; i < NCH; ++i) x[u][i] = rtk_load_piece<float, VEC>(v + vr * ld_v, i * 256 + lane * 4, c);
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
                for (int q = 0; q < 4; ++q) acc[i][q] = fmaf(g[u], rtk_bits_elem(x[u][i], q, 0.f), acc[i][q]);
        }
    }
    flush(key_next == cur);
}

// The runs that cross windows: the window where a run starts adds its slot-1 partial and the slot-0 partials of
// the following windows, in window order, and writes the destination row.
template <int NCH, bool VEC>
__global__ __launch_bounds__(256) void run_combine_kernel(const int32_t *__restrict__ skey, int64_t M, int64_t n_ent,
                                                             int c, float *__restrict__ gO, const float *__restrict__ P,
                                                             int64_t win) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * SC_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
        for (int q = 0; q < 4; ++q) acc[i][q] = P[(w * 2 + 1) * RTK_SCATTER_MAXC + i * 256 + lane * 4 + q];
    for (int64_t w2 = w + 1;; ++w2) {
        const float *src = P + (w2 * 2 + 0) * RTK_SCATTER_MAXC;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[i][q] += src[i * 256 + lane * 4 + q];
        const int64_t q1 = (w2 + 1) * win;
        if (q1 >= M || skey[q1] != e) break;
    }
    store_row<NCH, VEC>(gO + (int64_t)e * c, acc, c, lane);
}

// Where the pieces lie for M entries cut into windows of `win`.  P is carved for the shortest window any front end may
// use at this M, so the byte count depends on M alone.
struct ScatterPlan {
    int32_t *keys[2], *vals[2], *hist, *offs, *bs;
    float *P;
    int64_t M, ntiles, nh, nb, win, nwin;
    size_t total;
};
ScatterPlan carve(void *base, int64_t M, int64_t win) {
    ScatterPlan w;
    unsigned char *p = (unsigned char *)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char *q = p ? p + off : nullptr;
        off += rtk_align_up(bytes, 256);
        return q;
    };
    w.M = M;
    w.ntiles = rtk_cdiv(w.M, SC_TILE);
    w.nh = 256 * w.ntiles;
    w.nb = rtk_cdiv(w.nh, SCAN_BLK);
    w.win = win;
    w.nwin = rtk_cdiv(w.M, w.win);
    for (int i = 0; i < 2; ++i) {
        w.keys[i] = (int32_t *)take((size_t)w.M * 4);
        w.vals[i] = (int32_t *)take((size_t)w.M * 4);
    }
    w.hist = (int32_t *)take((size_t)w.nh * 4);
    w.offs = (int32_t *)take((size_t)w.nh * 4);
    w.bs = (int32_t *)take((size_t)(w.nb + 1) * 4);
    w.P = (float *)take((size_t)rtk_cdiv(w.M, rtk_scatter_window(w.M)) * 2 * RTK_SCATTER_MAXC * 4);
    w.total = off;
    return w;
}

unsigned key_blocks(int64_t M) { return (unsigned)(rtk_cdiv(M, 256) < 4096 ? rtk_cdiv(M, 256) : 4096); }

// The keys / vals of ws.keys[0], ws.vals[0] sorted by entity (stable), then the ordered sums into gO (zeroed by the caller).
// `owner` (flat lists, k = 1): entry i belongs to query owner[i]; null: to query i / k.  `ld_v`: the row pitch of v.
int sorted_scatter(const char *fn, const ScatterPlan &ws, int64_t n_ent, const float *dz, int64_t ld_dz, int64_t k,
                   const int32_t *owner, const float *v, int64_t ld_v, int c, float *gO, hipStream_t st) {
    const int64_t M = ws.M;
    int bits = 1;
    while ((n_ent >> bits) != 0) ++bits;             // keys are <= n_ent
    const unsigned tblocks = (unsigned)rtk_cdiv(ws.ntiles, SC_WAVES);
    int src = 0;
    for (int shift = 0; shift < bits; shift += 8, src ^= 1) {
        hipLaunchKernelGGL(sort_hist_kernel, dim3(tblocks), dim3(256), 0, st, ws.keys[src], M, shift, ws.ntiles, ws.hist);
        hipLaunchKernelGGL(scan_totals_kernel, dim3((unsigned)ws.nb), dim3(256), 0, st, ws.hist, ws.nh, ws.bs);
        hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, st, ws.bs, ws.nb);
        hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)ws.nb), dim3(256), 0, st, ws.hist, ws.nh, ws.bs, ws.offs);
        hipLaunchKernelGGL(sort_place_kernel, dim3(tblocks), dim3(256), 0, st, ws.keys[src], ws.vals[src], M, shift,
                           ws.ntiles, ws.offs, ws.keys[src ^ 1], ws.vals[src ^ 1]);
    }
    const bool vec = c % 4 == 0 && ld_v % 4 == 0 && ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(gO)) & 15) == 0;
    const unsigned wblocks = (unsigned)rtk_cdiv(ws.nwin, SC_WAVES);
    auto go = [&](auto nc, auto vc) {
        constexpr int NC = decltype(nc)::value;
        constexpr bool VC = decltype(vc)::value;
        RTK_LAUNCH_SCORE((run_sum_kernel<NC, VC>), dim3(wblocks), dim3(256), 0, st, ws.keys[src], ws.vals[src], M, n_ent,
                         dz, ld_dz, k, v, ld_v, c, gO, ws.P, ws.win, owner);
        hipLaunchKernelGGL((run_combine_kernel<NC, VC>), dim3(wblocks), dim3(256), 0, st, ws.keys[src], M, n_ent, c, gO,
                           ws.P, ws.win);
    };
    return rtk_dispatch_chunks<4>(fn, (c + 255) / 256, vec, go);
}

}  // namespace

size_t rtk_scatter_bytes(int64_t M) { return M <= 0 ? 0 : carve(nullptr, M, rtk_scatter_window(M)).total; }

int rtk_scatter_candidates(const char *fn, const int64_t *cand, int64_t ld_cand, int64_t batch, int64_t k, int64_t n_ent,
                           const float *dz, int64_t ld_dz, const float *v, int c, float *gO, void *workspace, hipStream_t st) {
    const int rc = rtk_zero_async(fn, gO, (size_t)n_ent * c * 4, st);
    const int64_t M = batch * k;
    if (rc != RTK_OK || M <= 0) return rc;
    const ScatterPlan ws = carve(workspace, M, rtk_scatter_window(M));
    hipLaunchKernelGGL(cand_keys_kernel, dim3(key_blocks(M)), dim3(256), 0, st, cand, ld_cand, k, n_ent, M, ws.keys[0], ws.vals[0]);
    return sorted_scatter(fn, ws, n_ent, dz, ld_dz, k, nullptr, v, c, c, gO, st);
}

int rtk_scatter_flat_ld(const char *fn, const int32_t *ent, const int32_t *owner, const float *dz, int64_t m, int64_t n_ent,
                        const float *v, int64_t ld_v, int c, float *gO, void *workspace, hipStream_t st) {
    const int rc = rtk_zero_async(fn, gO, (size_t)n_ent * c * 4, st);
    if (rc != RTK_OK || m <= 0) return rc;
    // m is the caller's BOUND on the entries (the surplus slots sort last and add nothing): the sums must not depend on
    // it, so the flat lists are always cut into the longest window, which P -- carved for rtk_scatter_window(m) -- holds
    const ScatterPlan ws = carve(workspace, m, RTK_SCATTER_WIN_MAX);
    hipLaunchKernelGGL(flat_keys_kernel, dim3(key_blocks(m)), dim3(256), 0, st, ent, n_ent, m, ws.keys[0], ws.vals[0]);
    return sorted_scatter(fn, ws, n_ent, dz, 1, 1, owner, v, ld_v, c, gO, st);
}

int rtk_scatter_flat(const char *fn, const int32_t *ent, const int32_t *owner, const float *dz, int64_t m, int64_t n_ent,
                     const float *v, int c, float *gO, void *workspace, hipStream_t st) {
    return rtk_scatter_flat_ld(fn, ent, owner, dz, m, n_ent, v, c, c, gO, workspace, st);
}
