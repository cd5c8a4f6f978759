// The ordered row scatter of the stage-1 backward (internal header): g[id, :] = sum over the queries d with that id of
// rows[d, :], for the subject rows and the relation rows in one launch.  Shared by the two forms of the stage-1 backward
// (rtk_query_bwd.hip, rtk_query_bwd_stream.hip): one text, so the same bits in both.
#pragma once
#include "rtk_common.h"

namespace {

__device__ __forceinline__ int64_t clamp_id(int64_t x, int64_t n) { return x < 0 ? 0 : (x >= n ? n - 1 : x); }

// Workgroups [0, B): subject rows -> gS;  [B, 2B): relation rows -> gR.  A workgroup whose query is
// not the first with its id exits; the first one sums the rows of all queries with that id, in
// increasing query order, and writes the destination row (the rest of the matrix was zeroed).
// The ids of the batch are copied to LDS once (B <= SC_IDS): the duplicate check and the match lists then
// cost no memory round trip -- read from global memory at every step the kernel was a chain of ~8 dependent
// latencies (34 us for 512 rows).
constexpr int SC_CB = 4;      // column blocks of 256 held in registers: row width <= 1024
constexpr int SC_IDS = 8192;  // ids kept in LDS (32 KB); larger batches read them from global memory
__global__ __launch_bounds__(256) void scatter_rows_kernel(const int64_t *__restrict__ sub_idx,
                                                           const float *__restrict__ rows_S, int b,
                                                           float *__restrict__ gS, int64_t n_sub,
                                                           const int64_t *__restrict__ rel_idx,
                                                           const float *__restrict__ rows_R, int a,
                                                           float *__restrict__ gR, int64_t n_rel, int B) {
    __shared__ unsigned long long masks[4];
    __shared__ int lst[256];
    __shared__ int sid[SC_IDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool rel = (int)blockIdx.x >= B;
    const int d = rel ? blockIdx.x - B : blockIdx.x;
    const int64_t *ids = rel ? rel_idx : sub_idx;
    const float *rows = rel ? rows_R : rows_S;
    float *dst = rel ? gR : gS;
    const int w = rel ? a : b;
    const int64_t n = rel ? n_rel : n_sub;        // < 2^31 (host)
    if (!dst) return;
    const bool in_lds = B <= SC_IDS;
    if (in_lds) {
        for (int i = t; i < B; i += 256) sid[i] = (int)clamp_id(ids[i], n);
        __syncthreads();
    }
    auto id_at = [&](int i) -> int { return in_lds ? sid[i] : (int)clamp_id(ids[i], n); };
    const int my = id_at(d);
    int dup = 0;
    for (int i = t; i < d; i += 256) dup |= (id_at(i) == my);
    if (__syncthreads_or(dup)) return;
    // Narrow rows (the relation rows: w = a = 10) leave 246 of the 256 threads idle and make the one workgroup of
    // a frequent relation the long pole (all 512 queries on one relation: 75 us; a WN18RR training batch: 36 us).
    // They are summed by `slots` = 256 / w groups of w threads: slot s adds list entries s, s + slots, ... in
    // that order, and the slot sums are added in slot order at the end -- a fixed shape, so still deterministic.
    const int slots = w <= 128 ? 256 / w : 1;
    const int slot = slots > 1 ? t / w : 0, scol = slots > 1 ? t - slot * w : 0;
    const bool sact = slots > 1 && slot < slots;
    float sacc = 0.f;
    float acc[SC_CB];
#pragma unroll
    for (int k = 0; k < SC_CB; ++k) acc[k] = 0.f;
    for (int base = d; base < B; base += 256) {
        // the queries of this block of 256 that carry the id, compacted in query order into lst[]
        const int i = base + t;
        const bool m = i < B && id_at(i) == my;
        const unsigned long long bal = __ballot(m);
        if (lane == 0) masks[wave] = bal;
        __syncthreads();
        int before = 0, count = 0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            const int pc = __popcll(masks[wv]);
            before += wv < wave ? pc : 0;
            count += pc;
        }
        if (m) lst[before + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        __syncthreads();
        if (slots > 1) {
            for (int j0 = slot; j0 < count; j0 += 8 * slots) {       // (uniform trip count per wave up to the guard)
                float x[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int j = j0 + q * slots;
                    x[q] = (sact && j < count) ? rows[(int64_t)lst[j] * w + scol] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (j0 + q * slots < count) sacc += x[q];
            }
        } else {
            // rows added in list (= query) order; the loads of eight rows are in flight together
            for (int j0 = 0; j0 < count; j0 += 8) {
                float x[8][SC_CB];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float *src = rows + (int64_t)lst[min(j0 + q, count - 1)] * w;
#pragma unroll
                    for (int k = 0; k < SC_CB; ++k) x[q][k] = (k * 256 + t < w) ? src[k * 256 + t] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (j0 + q < count) {
#pragma unroll
                        for (int k = 0; k < SC_CB; ++k) acc[k] += x[q][k];
                    }
            }
        }
        __syncthreads();
    }
    if (slots > 1) {
        float *part = reinterpret_cast<float *>(lst);        // 256 floats: slot sums, then added in slot order
        if (sact) part[t] = sacc;
        __syncthreads();
        if (t < w) {
            float sum = part[t];
            for (int sl = 1; sl < slots; ++sl) sum += part[sl * w + t];
            dst[(int64_t)my * w + t] = sum;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < SC_CB; ++k)
        if (k * 256 + t < w) dst[(int64_t)my * w + k * 256 + t] = acc[k];
}

}  // namespace
