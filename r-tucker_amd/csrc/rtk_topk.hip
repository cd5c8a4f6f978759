// Filtered top-k selection on the device: the k best candidates of every score row, best first, with the row's
// known-true objects removed (include/rtucker_hip.h, rtk_select_topk_*).  Tie rule of rtk_filtered_rank_f32 /
// torch.sort(descending=True, stable=True): higher score first, then lower entity id.
//
// One workgroup per row, the layout of filtered_rank_kernel (rtk_rank.hip); deterministic, integer LDS atomics only.
//  1. Keys: every value maps to an unsigned key whose integer order is the candidate order (-0 -> +0, every NaN -> one
//     NaN above +inf; bf16 rows keep 16-bit keys, so they compare as bf16).
//  2. Radix select on the keys, most significant digit first (11-bit digits: 11/11/10 for f32, 11/5 for bf16), over
//     the row's eligible columns: find K* with #(key > K*) < k' <= #(key >= K*), k' = min(k, #eligible).  As soon as
//     the digit bin that holds K* has at most TK_CAP candidates, one more sweep of the row copies that bin into LDS
//     (in column order) and everything above it straight into the result; the remaining digits and the final pass
//     read LDS.  So the row comes from global memory twice when the bin fits, once more per extra digit otherwise.
//  3. Collect: every key > K* (order irrelevant), then the first k' - #(key > K*) keys == K* in column order, from a
//     block-wide ordered count (per-wave __ballot + mbcnt, per-wave totals in LDS).  A row that ties throughout costs
//     one such ordered pass.
//  4. Bitonic sort of the k' (key, id) pairs in LDS (next_pow2(k') <= 1024 slots); values are written as float
//     (bf16 widens exactly), rows with fewer than k eligible candidates are padded with (-inf, -1).
// Exclusion: a bitmap of the row's known-true objects over a window of TK_WIN columns (the CSR segment walked once
// per window; rows of at most TK_WIN columns build it once), tested by every pass, so every count is of eligible
// columns only and an object listed twice is harmless.  Merge mode (an ids matrix instead of col0) tests a candidate
// id against the CSR segment directly; its rows are short.
#include "rtk_common.h"
#include "rtk_topk_key.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / RTK_WAVE;
constexpr int TK_U = 8;                        // columns per thread per chunk (loads in flight)
constexpr int TK_CHUNK = TK_THREADS * TK_U;
constexpr int TK_KMAX = 1024;
constexpr int TK_BINS = 2048;                  // 11-bit digits: 8 KiB of int32 counts
constexpr int TK_WIN = 1 << 16;                // exclusion-bitmap window, columns (8 KiB)
constexpr int TK_CAP = 4096;                   // LDS candidate list, entries (16 KiB keys + 16 KiB columns)
// LDS: 8 + 8 + 32 + 12 (sort buffer) + < 1 KiB = 60 KiB per workgroup: two workgroups per CU (160 KiB)

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// MERGE: candidate j of row d has id col_ids[d * ld_ids + j] (< 0: absent); otherwise id col0 + j
template <typename T, bool MERGE>
__global__ __launch_bounds__(TK_THREADS) void select_topk_kernel(
    const T *__restrict__ P, int n, int64_t ld, int64_t col0, const int64_t *__restrict__ col_ids, int64_t ld_ids,
    const int64_t *__restrict__ pair_slot, const int64_t *__restrict__ pair_ptr, const int64_t *__restrict__ pair_obj,
    const int64_t *__restrict__ keep_idx, int k, float *__restrict__ values_out, int64_t *__restrict__ ids_out) {
    constexpr int KB = 8 * (int)sizeof(T);
    constexpr int NPASS = KB == 32 ? 3 : 2;
    __shared__ int s_hist[TK_BINS];
    __shared__ uint32_t s_excl[TK_WIN / 32];
    __shared__ uint32_t s_lkey[TK_CAP];
    __shared__ int s_lcol[TK_CAP];
    __shared__ uint32_t s_skey[TK_KMAX];
    __shared__ int64_t s_sid[TK_KMAX];
    __shared__ int s_wcnt[2][TK_U][TK_WAVES];
    __shared__ int s_scan[TK_WAVES];
    __shared__ int s_misc[4];                  // bin, #above it, its count, sort-buffer append cursor

    const int d = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1), w = t / RTK_WAVE;
    const T *row = P + (int64_t)d * ld;
    const int64_t *rid = MERGE ? col_ids + (int64_t)d * ld_ids : nullptr;
    const int64_t s = pair_slot ? pair_slot[d] : -1;
    const int64_t keep = keep_idx ? keep_idx[d] : -1;
    const int64_t e_lo = s >= 0 ? pair_ptr[s] : 0, e_hi = s >= 0 ? pair_ptr[s + 1] : 0;
    const bool excl = e_hi > e_lo;
    const bool bitmap = !MERGE && excl;
    const int n_win = MERGE ? 1 : (n + TK_WIN - 1) / TK_WIN;

    for (int i = t; i < TK_KMAX; i += TK_THREADS) {
        s_skey[i] = 0u;
        s_sid[i] = INT64_MAX;
    }
    if (t == 0) s_misc[3] = 0;

    auto build_bitmap = [&](int wlo) {
        __syncthreads();                                   // the previous window's tests are done
        for (int i = t; i < TK_WIN / 32; i += TK_THREADS) s_excl[i] = 0u;
        __syncthreads();
        for (int64_t i = e_lo + t; i < e_hi; i += TK_THREADS) {
            const int64_t o = pair_obj[i];
            const int64_t j = o - col0;                    // ids outside this block are ignored
            if (o == keep || j < wlo || j >= n || j - wlo >= TK_WIN) continue;
            atomicOr(&s_excl[(j - wlo) >> 5], 1u << ((j - wlo) & 31));
        }
        __syncthreads();
    };
    auto merge_ok = [&](int64_t id) {
        if (id < 0) return false;
        if (excl && id != keep)
            for (int64_t i = e_lo; i < e_hi; ++i)
                if (pair_obj[i] == id) return false;
        return true;
    };
    auto id_of = [&](int col) -> int64_t { return MERGE ? rid[col] : col0 + col; };

    // body(key[U], ok[U], col[U]) once per chunk, by every thread (it may hold barriers); columns in row order
    bool built = false;                        // a row of one window builds its bitmap on the first sweep only
    auto sweep_global = [&](auto &&body) {
        for (int wi = 0; wi < n_win; ++wi) {
            const int wlo = wi * TK_WIN, whi = MERGE ? n : min(n, wlo + TK_WIN);
            if (bitmap && (n_win > 1 || !built)) {
                build_bitmap(wlo);
                built = true;
            }
            for (int base = wlo; base < whi; base += TK_CHUNK) {
                T x[TK_U];
                int64_t idv[TK_U];
#pragma unroll
                for (int u = 0; u < TK_U; ++u) {
                    const int j = base + u * TK_THREADS + t;
                    x[u] = j < whi ? row[j] : T(0);
                    if (MERGE) idv[u] = j < whi ? rid[j] : -1;
                }
                uint32_t key[TK_U];
                bool ok[TK_U];
                int col[TK_U];
#pragma unroll
                for (int u = 0; u < TK_U; ++u) {
                    const int j = base + u * TK_THREADS + t;
                    col[u] = j;
                    key[u] = sel_key(x[u]);
                    ok[u] = j < whi && (MERGE ? merge_ok(idv[u]) : !(bitmap && (s_excl[(j - wlo) >> 5] >> ((j - wlo) & 31) & 1u)));
                }
                body(key, ok, col);
            }
        }
    };
    auto sweep_list = [&](int n_list, auto &&body) {
        for (int base = 0; base < n_list; base += TK_CHUNK) {
            uint32_t key[TK_U];
            bool ok[TK_U];
            int col[TK_U];
#pragma unroll
            for (int u = 0; u < TK_U; ++u) {
                const int i = base + u * TK_THREADS + t;
                ok[u] = i < n_list;
                key[u] = ok[u] ? s_lkey[i] : 0u;
                col[u] = ok[u] ? s_lcol[i] : 0;
            }
            body(key, ok, col);
        }
    };
    // positions (within the chunk, in column order) of the flagged columns; returns the chunk's total.  The per-wave
    // counts are double-buffered: a wave can be one chunk ahead, never two (the barrier)
    int cbuf = 0;
    auto ordered = [&](const bool(&f)[TK_U], int(&pos)[TK_U]) {
        unsigned long long m[TK_U];
#pragma unroll
        for (int u = 0; u < TK_U; ++u) {
            m[u] = __ballot(f[u]);
            if (lane == 0) s_wcnt[cbuf][u][w] = __popcll(m[u]);
        }
        __syncthreads();
        int run = 0;
#pragma unroll
        for (int u = 0; u < TK_U; ++u)
#pragma unroll
            for (int v = 0; v < TK_WAVES; ++v) {
                if (v == w) pos[u] = run + lanes_below(m[u]);
                run += s_wcnt[cbuf][u][v];
            }
        cbuf ^= 1;
        return run;
    };
    auto append_sorted = [&](uint32_t key, int col, int cap) {
        const int q = atomicAdd(&s_misc[3], 1);
        if (q < cap) {
            s_skey[q] = key;
            s_sid[q] = id_of(col);
        }
    };

    uint32_t prefix = 0u;
    int kp = 0, k_rem = 0, n_list = -1;        // n_list >= 0: the candidates are in LDS
    for (int p = 0; p < NPASS; ++p) {
        const int sh = KB == 32 ? (p == 0 ? 21 : p == 1 ? 10 : 0) : (p == 0 ? 5 : 0);
        const int hi = KB == 32 ? (p == 0 ? 32 : p == 1 ? 21 : 10) : (p == 0 ? 16 : 5);
        const uint32_t dmask = (1u << (hi - sh)) - 1u;
        for (int i = t; i < TK_BINS; i += TK_THREADS) s_hist[i] = 0;
        __syncthreads();
        auto hist = [&](const uint32_t(&key)[TK_U], const bool(&ok)[TK_U], const int(&)[TK_U]) {
#pragma unroll
            for (int u = 0; u < TK_U; ++u)
                if (ok[u] && (hi >= 32 || (key[u] >> hi) == (prefix >> hi))) atomicAdd(&s_hist[(key[u] >> sh) & dmask], 1);
        };
        if (n_list >= 0) sweep_list(n_list, hist);
        else sweep_global(hist);
        __syncthreads();
        // the bin holding the want-th best candidate: thread t owns bins [TK_BINS - 8 (t + 1), TK_BINS - 8 t), top down
        constexpr int PER = TK_BINS / TK_THREADS;
        const int b0 = TK_BINS - PER * (t + 1);
        int loc[PER], sum = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) sum += (loc[i] = s_hist[b0 + PER - 1 - i]);
        int incl = sum;
#pragma unroll
        for (int o = 1; o < RTK_WAVE; o <<= 1) {
            const int y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == RTK_WAVE - 1) s_scan[w] = incl;
        __syncthreads();
        int run = incl - sum, total = 0;
#pragma unroll
        for (int v = 0; v < TK_WAVES; ++v) {
            total += s_scan[v];
            if (v < w) run += s_scan[v];
        }
        if (p == 0) kp = k_rem = min(k, total);
        if (kp == 0) break;                                // no eligible column: the row is all padding
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (run < k_rem && k_rem <= run + loc[i]) {
                s_misc[0] = b0 + PER - 1 - i;
                s_misc[1] = run;
                s_misc[2] = loc[i];
            }
            run += loc[i];
        }
        __syncthreads();
        const int b = s_misc[0], above = s_misc[1], cnt_b = s_misc[2];
        k_rem -= above;
        prefix |= (uint32_t)b << sh;
        if (n_list < 0 && p + 1 < NPASS && cnt_b <= TK_CAP) {
            // the bin into LDS in column order; the bins above it are selected outright (fewer than k')
            const int cap = kp - k_rem;
            int got = 0;
            sweep_global([&](const uint32_t(&key)[TK_U], const bool(&ok)[TK_U], const int(&col)[TK_U]) {
                bool f[TK_U];
                int pos[TK_U];
#pragma unroll
                for (int u = 0; u < TK_U; ++u) {
                    f[u] = ok[u] && (key[u] >> sh) == (prefix >> sh);
                    if (ok[u] && (key[u] >> sh) > (prefix >> sh)) append_sorted(key[u], col[u], cap);
                }
                const int tot = ordered(f, pos);
#pragma unroll
                for (int u = 0; u < TK_U; ++u)
                    if (f[u] && got + pos[u] < TK_CAP) {
                        s_lkey[got + pos[u]] = key[u];
                        s_lcol[got + pos[u]] = col[u];
                    }
                got += tot;
            });
            n_list = min(got, TK_CAP);
            __syncthreads();
        }
    }

    if (kp > 0) {
        // collect: key > K* anywhere (the append cursor continues after the bins taken above), the first k_rem keys
        // == K* in column order into the slots after them
        const uint32_t kstar = prefix;
        const int n_gt = kp - k_rem;
        int got = 0;
        auto collect = [&](const uint32_t(&key)[TK_U], const bool(&ok)[TK_U], const int(&col)[TK_U]) {
            bool f[TK_U];
            int pos[TK_U];
#pragma unroll
            for (int u = 0; u < TK_U; ++u) {
                f[u] = ok[u] && key[u] == kstar;
                if (ok[u] && key[u] > kstar) append_sorted(key[u], col[u], n_gt);
            }
            const int tot = ordered(f, pos);
#pragma unroll
            for (int u = 0; u < TK_U; ++u)
                if (f[u] && got + pos[u] < k_rem) {
                    s_skey[n_gt + got + pos[u]] = key[u];
                    s_sid[n_gt + got + pos[u]] = id_of(col[u]);
                }
            got += tot;
        };
        if (n_list >= 0) sweep_list(n_list, collect);
        else sweep_global(collect);
        __syncthreads();
        // bitonic sort, best first: (key desc, id asc); the padding slots (key 0, id max) sort last
        int p2 = 1;
        while (p2 < kp) p2 <<= 1;
        for (int size = 2; size <= p2; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int i = t; i < p2 / 2; i += TK_THREADS) {
                    const int a = 2 * i - (i & (stride - 1)), c = a + stride;
                    const uint32_t ka = s_skey[a], kc = s_skey[c];
                    const int64_t ia = s_sid[a], ic = s_sid[c];
                    const bool c_better = kc > ka || (kc == ka && ic < ia);
                    const bool a_better = ka > kc || (ka == kc && ia < ic);
                    if ((a & size) == 0 ? c_better : a_better) {
                        s_skey[a] = kc;
                        s_skey[c] = ka;
                        s_sid[a] = ic;
                        s_sid[c] = ia;
                    }
                }
                __syncthreads();
            }
    }
    for (int i = t; i < k; i += TK_THREADS) {
        const bool real = i < kp && s_skey[i] != 0u;
        values_out[(int64_t)d * k + i] = real ? sel_value(s_skey[i], T()) : -INFINITY;
        ids_out[(int64_t)d * k + i] = real ? s_sid[i] : -1;
    }
}

template <typename T>
int select_topk(const char *what, const T *P, int64_t batch, int64_t n_cols, int64_t ld, int64_t col0,
                const int64_t *col_ids, int64_t ld_ids, const int64_t *pair_slot, const int64_t *pair_ptr,
                const int64_t *pair_obj, const int64_t *keep_idx, int k, float *values_out, int64_t *ids_out,
                void *workspace, size_t workspace_bytes, void *stream) {
    RTK_REQUIRE(P && values_out && ids_out, RTK_ERR_BAD_ARG, "%s: null operand", what);
    RTK_REQUIRE(k >= 1 && k <= TK_KMAX, RTK_ERR_BAD_ARG, "%s: k = %d outside [1, %d]", what, k, TK_KMAX);
    RTK_REQUIRE(batch >= 0 && n_cols >= 0 && ld >= n_cols && col0 >= 0, RTK_ERR_BAD_ARG,
                "%s: bad sizes (batch %lld, n_cols %lld, ld %lld, col0 %lld)", what, (long long)batch,
                (long long)n_cols, (long long)ld, (long long)col0);
    RTK_REQUIRE(!col_ids || ld_ids >= n_cols, RTK_ERR_BAD_ARG, "%s: ld_ids < n_cols", what);
    RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", what);
    RTK_REQUIRE(workspace_bytes >= rtk_select_topk_workspace_bytes(batch, n_cols, k), RTK_ERR_WORKSPACE,
                "%s: workspace too small", what);
    RTK_REQUIRE(batch < (1ll << 31) && n_cols < (1ll << 31) - TK_CHUNK, RTK_ERR_UNSUPPORTED, "%s: dimension too large", what);
    if (batch == 0) return RTK_OK;
    (void)workspace;
    if (col_ids)
        hipLaunchKernelGGL((select_topk_kernel<T, true>), dim3((unsigned)batch), dim3(TK_THREADS), 0, (hipStream_t)stream,
                           P, (int)n_cols, ld, col0, col_ids, ld_ids, pair_slot, pair_ptr, pair_obj, keep_idx, k,
                           values_out, ids_out);
    else
        hipLaunchKernelGGL((select_topk_kernel<T, false>), dim3((unsigned)batch), dim3(TK_THREADS), 0, (hipStream_t)stream,
                           P, (int)n_cols, ld, col0, col_ids, ld_ids, pair_slot, pair_ptr, pair_obj, keep_idx, k,
                           values_out, ids_out);
    return rtk_check_launch(what);
}

}  // namespace

extern "C" size_t rtk_select_topk_workspace_bytes(int64_t batch, int64_t n_cols, int k) {
    (void)batch, (void)n_cols, (void)k;
    return 0;                                  // every row is selected in its workgroup's LDS
}

extern "C" int rtk_select_topk_f32(const float *P, int64_t batch, int64_t n_cols, int64_t ld, int64_t col0,
                                   const int64_t *col_ids, int64_t ld_ids, const int64_t *pair_slot,
                                   const int64_t *pair_ptr, const int64_t *pair_obj, const int64_t *keep_idx, int k,
                                   float *values_out, int64_t *ids_out, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    return select_topk("rtk_select_topk_f32", P, batch, n_cols, ld, col0, col_ids, ld_ids, pair_slot, pair_ptr, pair_obj,
                       keep_idx, k, values_out, ids_out, workspace, workspace_bytes, stream);
}

extern "C" int rtk_select_topk_bf16(const uint16_t *P, int64_t batch, int64_t n_cols, int64_t ld, int64_t col0,
                                    const int64_t *col_ids, int64_t ld_ids, const int64_t *pair_slot,
                                    const int64_t *pair_ptr, const int64_t *pair_obj, const int64_t *keep_idx, int k,
                                    float *values_out, int64_t *ids_out, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    return select_topk("rtk_select_topk_bf16", (const rtk_bf16 *)P, batch, n_cols, ld, col0, col_ids, ld_ids, pair_slot,
                       pair_ptr, pair_obj, keep_idx, k, values_out, ids_out, workspace, workspace_bytes, stream);
}
