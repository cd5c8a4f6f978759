// What the matrix-free training losses share (rtk_bce_stream.hip, rtk_ce_stream.hip, rtk_bce_stream_bf16.hip; internal
// header): the two sweeps and the positives' kernel as skeletons that take the loss's link function as a policy, the
// transposed operand images of the second tile product, the flat lists of the positives and the workspace pieces common
// to them.  The sweeps here are the fp32 ones; rtk_stream_bf16_kernel.h has those of bf16 entity rows, which share
// pos_kernel, pack_v_kernel, go_prologue and the workspace layout.
//
//   rows_sweep    sweep 1.  The score tile is computed with the QUERY on the lane and the entities in the accumulator
//                 registers (entity fragments as the A operand, the packed query planes as B), so the 32 x 32 tile of x is
//                 the A operand of the next product, dv[d, :] += sum_j x[d, j] O[j, :], with no lane movement.
//   GoSweep       sweep 2, the entity-stationary sweep of rtk_score_rank_kernel.h: gO[j, :] += sum_d x[d, j] (s v[d, :]).
//   pos_kernel    the positives: one workgroup per query re-scores the query's CSR entries with Frag (the sweeps' bits).
//
// Both tile products are three f16 MFMAs per k-step on hi/lo halves (x scaled by 2^14; O and s v by a power of two from
// their largest magnitude), accumulated in fp32.  No float atomics: every sum has a fixed order.
#pragma once
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_rank_kernel.h"
#include "rtk_scatter.h"
#include "rtk_score_select.h"

namespace {

constexpr int BS_WAVES = SW_WAVES;
constexpr int BS_MAX_KS = SW_MAX_KS_F32;       // Frag<float, KS>'s range: c <= 208
constexpr int BS_POS_Y = 4;                    // loss partials per query of pos_kernel (one per wave)
constexpr float BS_X_UP = 16384.0f;            // |x| <= 1 scaled to 2^14 before the hi/lo split

__host__ __device__ constexpr int nct_of(int ks) { return (ks + 1) / 2; }       // 32-column tiles of 16 ks columns
// bytes of the transposed image of a 32-row tile: [plane][column tile][k-step][lane][8 halves]
__host__ __device__ constexpr int timg_bytes(int ks) { return nct_of(ks) * 4096; }

// index, in halves, of element (row j of the tile, column col) in plane 0 of the transposed image: lane (col & 31, h)
// holds in k-step t the rows 16 t + 8 (q >> 2) + 4 h + (q & 3), q = 0..7 -- the order in which an accumulator tile
// supplies its rows as an operand
__device__ __forceinline__ int timg_index(int j, int col) {
    const int t = j >> 4, q = ((j >> 3) & 1) * 4 + (j & 3), h = (j >> 2) & 1;
    return ((((col >> 5) * 2 + t) * 64) + h * 32 + (col & 31)) * 8 + q;
}

__device__ __forceinline__ f32x16 zero16() {
    return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// the 16 values of a tile held by a lane, scaled and split into the two k-steps' operand fragments
__device__ __forceinline__ void split_x(const float (&x)[16], f16x8 (&xh)[2], f16x8 (&xl)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float y = x[8 * t + q] * BS_X_UP;
            const _Float16 hi = (_Float16)y;
            xh[t][q] = hi;
            xl[t][q] = (_Float16)(y - (float)hi);
        }
}

// acc[ct] += X * T for the transposed image `timg` (plane stride in 16-byte units: NCT * 128)
template <int NCT>
__device__ __forceinline__ void tile_product(const f16x8 (&xh)[2], const f16x8 (&xl)[2], const f16x8 *__restrict__ timg,
                                             int lane, f32x16 (&acc)[NCT]) {
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f16x8 bh = timg[(ct * 2 + t) * 64 + lane], bl = timg[(NCT * 2 + ct * 2 + t) * 64 + lane];
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[t], bh, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[t], bl, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl[t], bh, acc[ct], 0, 0, 0);
        }
}

template <int KS>
struct RowsLds {
    static constexpr int NCT = nct_of(KS);
    static constexpr int A1 = 0;                       // [2][KS][64] x 16 B: the tile's rows as the chain's operand
    static constexpr int T2 = 2 * KS * 1024;           // the transposed image of the same rows (one scale for all of O)
    static constexpr int KC = T2 + timg_bytes(KS);     // 32 floats: Frag's kcol of the rows
    static constexpr int TOTAL = KC + 128;
};

// Sweep 1, the skeleton.  Workgroup (qg, sp): query tiles 4 qg .. 4 qg + 3 (one per wave), entity tiles of split sp.
// Each 32-row entity tile is converted once per workgroup into LDS (RowsLds); a wave scores it against its query tile
// with Frag::chain's products, the roles swapped: element e of the accumulator is entity row 8 (e / 4) + 4 h + e % 4 of
// the tile, query r of the wave.  What is done with the 16 values is the policy's (the link function of the loss):
//
//   begin(d, on)                      before the sweep; d is the lane's query, `on` whether its tile exists
//   tile(acc, srow, kc, tile, h, N, x)  the accumulators of one entity tile with the query's row factor and the tile's
//                                     32 column factors (LDS); fills x, the tile of the logit gradient (DV only)
//   finish(sp, d, h, B)               after the sweep: the policy's partial results of split sp
//
// With DV the tile of x is the A operand of dv[d, :] += sum_j x[d, j] O[j, :]; the slabs go out per split.
template <int KS, int SG, bool DV, typename P>
__device__ __forceinline__ void rows_sweep(P &pol, const unsigned char *__restrict__ qp, int B, const float *__restrict__ O,
                                           int N, int c, const float *__restrict__ o_bound, int n_splits,
                                           float *__restrict__ slab) {
    typedef RowsLds<KS> L;
    constexpr int NCT = L::NCT, CP = 32 * NCT;
    constexpr int NF = (4 * KS + 7) / 8;               // float4 pieces of a row per staging thread
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int qg = (int)blockIdx.x / n_splits, sp = (int)blockIdx.x % n_splits;
    const int n_mt = (B + 31) >> 5, n_t = (N + 31) >> 5;
    const int mt = qg * BS_WAVES + wave;
    const bool active = mt < n_mt;                                  // (wave-uniform)
    const int tb = (int)((int64_t)n_t * sp / n_splits), te = (int)((int64_t)n_t * (sp + 1) / n_splits);

    f16x8 Qh[KS], Ql[KS];
    float srow = 1.0f;
    if (active) {
        load_a<float, KS>(qp, mt, r, h, Qh, Ql);
        srow = reinterpret_cast<const float *>(qp + mt * tile_bytes<float, KS>())[r];
    } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Qh[ks] = Ql[ks] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    pol.begin(mt * 32 + r, active);
    f32x16 dacc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) dacc[ct] = zero16();
    const float up2 = DV ? ldexpf(1.0f, rtk_pack_shift(o_bound[0])) : 1.0f;

    // staging: 8 consecutive threads take one row, thread `part` the float4 pieces part, part + 8, ...
    const int srw = t >> 3, part = t & 7;
    f32x4 stg[NF];
    auto stage_load = [&](int tile) {
        const float *row = O + (int64_t)min(tile * 32 + srw, N - 1) * c;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int k0 = 4 * (part + 8 * i);
            stg[i] = (k0 + 4 <= c) ? *reinterpret_cast<const f32x4 *>(row + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stage_store = [&]() {
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) mx = fmaxf(mx, fabsf(stg[i][q]));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        mx = fmaxf(mx, __shfl_xor(mx, 4));
        float up, kc;
        Frag<float, KS>::template row_scale<SG>(mx, up, kc);
        if (part == 0) reinterpret_cast<float *>(lds + L::KC)[srw] = kc;
        _Float16 *t2 = reinterpret_cast<_Float16 *>(lds + L::T2);
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int f = part + 8 * i;
            if (f >= 4 * KS) continue;
            const int ks = f >> 2, hh = (f >> 1) & 1, q0 = (f & 1) * 4;
            f16x4 hi, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float y = stg[i][q] * up;
                const _Float16 y0 = (_Float16)y;
                hi[q] = y0;
                lo[q] = (_Float16)(y - (float)y0);
            }
            const int at = (ks * 64 + hh * 32 + srw) * 16 + q0 * 2;
            *reinterpret_cast<f16x4 *>(lds + L::A1 + at) = hi;
            *reinterpret_cast<f16x4 *>(lds + L::A1 + KS * 1024 + at) = lo;
            if (DV) {                                               // (columns past 16 KS stay unwritten: they feed output columns >= c, never stored)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float y = stg[i][q] * up2;
                    const _Float16 y0 = (_Float16)y;
                    const int ix = timg_index(srw, 4 * f + q);
                    t2[ix] = y0;
                    t2[NCT * 1024 + ix] = (_Float16)(y - (float)y0);
                }
            }
        }
    };

    if (tb < te) stage_load(tb);
    for (int tile = tb; tile < te; ++tile) {
        stage_store();
        __syncthreads();
        if (tile + 1 < te) stage_load(tile + 1);
        if (active) {
            const f16x8 *la = reinterpret_cast<const f16x8 *>(lds + L::A1);
            f32x16 acc;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {                       // Frag::chain's products with the roles swapped
                const f16x8 eh = la[ks * 64 + lane], el = la[(KS + ks) * 64 + lane];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(eh, Qh[ks], ks == 0 ? zero16() : acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(el, Qh[ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(eh, Ql[ks], acc, 0, 0, 0);
            }
            float x[16];
            pol.tile(acc, srow, lds + L::KC, tile, h, N, x);
            if (DV) {
                f16x8 xh[2], xl[2];
                split_x(x, xh, xl);
                tile_product<NCT>(xh, xl, reinterpret_cast<const f16x8 *>(lds + L::T2), lane, dacc);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    pol.finish(sp, mt * 32 + r, h, B);
    if (DV) {
        // element e of dacc[ct]: query row 8 (e / 4) + 4 h + e % 4 of the tile, column 32 ct + r
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int dq = mt * 32 + acc_row(e, h);
                if (dq < B) slab[((int64_t)sp * B + dq) * CP + ct * 32 + r] = dacc[ct][e];
            }
    }
}

// dv[d, :] = (the splits' slabs, in split order) * 2^-(14 + sh_O) + the positives' share; thread t: column t
__device__ __forceinline__ void finish_dv_row(int d, int t, int B, int c, int cp, int n_splits,
                                              const float *__restrict__ slab, const float *__restrict__ dvpos,
                                              const float *__restrict__ o_bound, float *__restrict__ dv) {
    if (dv && t < c) {
        const float un = ldexpf(1.0f, -14 - rtk_pack_shift(o_bound[0]));
        float s = 0.f;
        for (int k = 0; k < n_splits; ++k) s += slab[((int64_t)k * B + d) * cp + t];
        dv[(int64_t)d * c + t] = s * un + dvpos[(int64_t)d * c + t];
    }
}

// off[d] = entries of the queries before d in the flat lists (exclusive prefix of the CSR list lengths), off[B] = all.
__global__ __launch_bounds__(256) void pos_offsets_kernel(int B, const int64_t *__restrict__ pair_slot,
                                                          const int64_t *__restrict__ pair_ptr, int64_t max_pos,
                                                          int32_t *__restrict__ off, uint32_t *__restrict__ err) {
    __shared__ long long wsum[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    long long carry = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int d = b0 + t;
        long long len = 0;
        if (d < B) {
            const int64_t s = pair_slot[d];
            if (s >= 0) len = pair_ptr[s + 1] - pair_ptr[s];
            if (len < 0) len = 0;
        }
        long long inc = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(inc, o);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        long long before = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            before += i < wv ? wsum[i] : 0;
            tot += wsum[i];
        }
        __syncthreads();
        const long long ex = carry + before + inc - len;
        if (d < B) off[d] = (int32_t)(ex < max_pos ? ex : max_pos);
        carry += tot;
    }
    if (t == 0) {
        off[B] = (int32_t)(carry < max_pos ? carry : max_pos);
        if (carry > max_pos) atomicOr(err, 8u);                   // the lists are longer than the caller's bound
    }
}

__global__ __launch_bounds__(256) void pos_fill_kernel(int64_t m, int32_t n_ent, int32_t *__restrict__ ent,
                                                       int32_t *__restrict__ owner, float *__restrict__ dzf) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        ent[i] = n_ent;                                           // no entity: adds nothing
        owner[i] = 0;
        dzf[i] = 0.f;
    }
}

// The positives of query d = blockIdx.x: wave w takes the CSR entries [i0 + 32 (w + 4 k), + 32), one per column of a
// tile whose rows are all query d (filter_kernel's form).  pair_obj holds global ids; the block owns col0 <= id < col0 + N
// (local row id - col0), every other entry is skipped.  The link LK says what an entry adds:
//
//   coef(dt, n)                             the weight of one entry of a list of n (dt = 1 - eps)
//   term<SG>(f, acc, srow, coef, lacc, dz)  from the accumulated value of the entry (row factor srow, column factor in
//                                           f): its loss term, added to lacc, and its logit gradient dz
// T: the operand type of O and of the packed planes; the dv share covers 64 lanes x 4 columns (fp32, c <= 208) or
// x 8 (bf16, c <= 512; the vector row path: c % 8 == 0, O 16-byte aligned).
template <typename T, int KS, int SG, typename LK>
__global__ __launch_bounds__(64 * BS_WAVES) void pos_kernel(const unsigned char *__restrict__ qp, int B,
                                                            const T *__restrict__ O, int N, int col0, int c, float dt,
                                                            const int64_t *__restrict__ pair_slot,
                                                            const int64_t *__restrict__ pair_ptr,
                                                            const int64_t *__restrict__ pair_obj,
                                                            double *__restrict__ rows_pos, float *__restrict__ dvpos,
                                                            const int32_t *__restrict__ off, int64_t max_pos,
                                                            int32_t *__restrict__ ent, int32_t *__restrict__ owner,
                                                            float *__restrict__ dzf) {
    constexpr int NDV = sizeof(T) == 4 ? 4 : 8;
    __shared__ float part[BS_WAVES][64 * NDV];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = blockIdx.x;
    const int64_t s = pair_slot[d];
    const int64_t i0 = s >= 0 ? pair_ptr[s] : 0, i1 = s >= 0 ? pair_ptr[s + 1] : 0;
    const float coef = LK::coef(dt, i1 - i0);
    float lacc = 0.f;
    float dva[NDV];
#pragma unroll
    for (int k = 0; k < NDV; ++k) dva[k] = 0.f;
    if (i0 + 32 * wave < i1) {
        QueryRow<T, KS> q;
        q.load(qp, d, h);
        Frag<T, KS> f;
        for (int64_t base = i0 + 32 * wave; base < i1; base += 32 * BS_WAVES) {       // wave-uniform
            const int64_t i = base + r;
            const int64_t jr = i < i1 ? pair_obj[i] - col0 : -1;     // local row
            const bool ok = jr >= 0 && jr < N;
            float dz = 0.f;
            if (__ballot(ok) != 0) {
                f.load(O, ok ? jr : 0, c, h, true);                // QueryRow::score up to the link
                f.template convert<SG>();
                const f32x16 acc = f.chain(q.A0, q.A1);
                if (h == 0 && ok)                                  // element 0 of lane r: row 0, column r
                    LK::template term<SG>(f, acc[0], q.srow, coef, lacc, dz);
            }
            if (off && h == 0 && i < i1) {
                const int64_t at = (int64_t)off[d] + (i - i0);
                if (at < max_pos) {
                    ent[at] = ok ? (int32_t)jr : N;
                    owner[at] = d;
                    dzf[at] = dz;
                }
            }
            if (dvpos) {
                for (int rr = 0; rr < 32; ++rr) {
                    const float g = __shfl(dz, rr);
                    const int j = __shfl((int)(ok ? jr : 0), rr);
                    if (g != 0.f) {                                // (uniform)
                        const T *oj = O + (int64_t)j * c;
#pragma unroll
                        for (int k = 0; k < NDV; ++k)
                            if (lane + 64 * k < c) dva[k] = fmaf(g, rtk_to_f32(oj[lane + 64 * k]), dva[k]);
                    }
                }
            }
        }
    }
    if (rows_pos) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lacc += __shfl_xor(lacc, o);
        if (lane == 0) rows_pos[(int64_t)d * BS_POS_Y + wave] = -(double)lacc;
    }
    if (dvpos) {
#pragma unroll
        for (int k = 0; k < NDV; ++k) part[wave][lane + 64 * k] = dva[k];
        __syncthreads();
#pragma unroll
        for (int col = threadIdx.x; col < 64 * NDV; col += 64 * BS_WAVES)
            if (col < c) dvpos[(int64_t)d * c + col] = ((part[0][col] + part[1][col]) + part[2][col]) + part[3][col];
    }
}

// vs = scale * v (the small operand of gO carries g / (B N))
__global__ __launch_bounds__(256) void scale_v_kernel(const float *__restrict__ v, int64_t n, const float *__restrict__ scale,
                                                      float *__restrict__ vs) {
    const float s = scale[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) vs[i] = v[i] * s;
}

// the transposed images of vs, one per query tile, scaled by the power of two of its largest magnitude
__global__ __launch_bounds__(256) void pack_v_kernel(const float *__restrict__ vs, int B, int c, int nct,
                                                     const float *__restrict__ v_bound, _Float16 *__restrict__ vp) {
    const int mt = blockIdx.x, cp = 32 * nct;
    const float up = ldexpf(1.0f, rtk_pack_shift(v_bound[0]));
    _Float16 *img = vp + (int64_t)mt * nct * 2048;
    for (int i = threadIdx.x; i < 32 * cp; i += 256) {
        const int j = i / cp, col = i - j * cp, d = mt * 32 + j;
        const float y = (d < B && col < c) ? vs[(int64_t)d * c + col] * up : 0.f;
        const _Float16 hi = (_Float16)y;
        const int ix = timg_index(j, col);
        img[ix] = hi;
        img[nct * 1024 + ix] = (_Float16)(y - (float)hi);
    }
}

// LDS of sweep 2: the packed query tile, the tile's image of s v behind it and QB bytes of per-query values of the link
template <int KS, int QB = 0>
struct GoLds {
    static constexpr int TILE = (int)tile_bytes<float, KS>();      // the packed query tile (header + two planes)
    static constexpr int IMG = timg_bytes(KS);                     // ... the tile's image of s v behind it
    static constexpr int EXTRA = IMG + QB;                         // ... and the link's values of the 32 queries
    static constexpr int TOTAL = 2 * (TILE + EXTRA);
};

// What go_kernel does with the sweep: the tile of x is the A operand of X^T V against the image of s v that travels
// with the query tile; a wave's 32 rows of gO are accumulated over the query tiles and stored once per entity tile.
// The link LK turns an accumulated value into x:
//
//   QB                         bytes per query tile that travel with it (qx + mt * QB; a multiple of 16, at most 4096)
//   rows4(q4, rw)              fetch what the link needs of query rows rw .. rw + 3 from the staged bytes q4
//   x<SG>(f, acc, srow, q, valid)   x of query row rw + q against the fragment's entity
template <int KS, int SG, typename LK>
struct GoSweep {
    static constexpr int NCT = nct_of(KS);
    static constexpr int IMG = GoLds<KS>::IMG, EXTRA = IMG + LK::QB;
    static constexpr int NLV = IMG / 16 / (64 * BS_WAVES);          // 16-byte pieces of the image per thread: NCT
    static_assert(IMG % (16 * 64 * BS_WAVES) == 0, "the image of s v is staged without a bound: whole pieces per thread");
    static_assert(LK::QB % 16 == 0 && LK::QB <= 16 * 64 * BS_WAVES, "the link's values: at most one piece per thread");
    const unsigned char *__restrict__ vp;
    const unsigned char *__restrict__ qx;
    int B, N, c;
    float un;
    LK lk;
    float *__restrict__ gO;
    u32x4 vstg[NLV];
    u32x4 qstg;
    f32x16 gacc[NCT];

    __device__ __forceinline__ void load_extra(SweepLane ln, int mt) {
        const u32x4 *sv = reinterpret_cast<const u32x4 *>(vp + (int64_t)mt * IMG);
#pragma unroll
        for (int i = 0; i < NLV; ++i) vstg[i] = sv[i * 64 * BS_WAVES + ln.t];
        if (LK::QB > 0 && ln.t < LK::QB / 16) qstg = reinterpret_cast<const u32x4 *>(qx + (int64_t)mt * LK::QB)[ln.t];
    }
    __device__ __forceinline__ void store_extra(SweepLane ln, int extra) const {
        u32x4 *dst = reinterpret_cast<u32x4 *>(sweep_lds + extra);
#pragma unroll
        for (int i = 0; i < NLV; ++i) dst[i * 64 * BS_WAVES + ln.t] = vstg[i];
        if (LK::QB > 0 && ln.t < LK::QB / 16) reinterpret_cast<u32x4 *>(sweep_lds + extra + IMG)[ln.t] = qstg;
    }
    __device__ __forceinline__ void begin_tile() {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) gacc[ct] = zero16();
    }
    // element e: query row acc_row(e, h) of the tile, entity r of the wave
    __device__ __forceinline__ void score(SweepLane ln, const Frag<float, KS> &f, const f32x16 &acc,
                                          const unsigned char *buf, int, int, bool, int mt) {
        float x[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rw = acc_row(4 * g, ln.h);
            const f32x4 sr4 = *reinterpret_cast<const f32x4 *>(buf + rw * 4);
            lk.rows4(buf + GoLds<KS>::TILE + IMG, rw);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                x[4 * g + q] = lk.template x<SG>(f, acc[4 * g + q], sr4[q], q, mt * 32 + rw + q < B);
        }
        f16x8 xh[2], xl[2];
        split_x(x, xh, xl);
        tile_product<NCT>(xh, xl, reinterpret_cast<const f16x8 *>(buf + GoLds<KS>::TILE), ln.lane, gacc);
    }
    __device__ __forceinline__ void publish(SweepLane, int, int, int, int, int, bool) const {}
    // element e of gacc[ct]: entity row acc_row(e, h) of the wave, column 32 ct + r; on top of the positives' share
    // that the ordered scatter wrote
    __device__ __forceinline__ void end_tile(SweepLane ln, int tile) const {
        const int j0 = tile * SW_TILE + ln.wave * 32;                // the wave's first row
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int col = ct * 32 + ln.r;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = j0 + acc_row(e, ln.h);
                if (j < N && col < c) {
                    float *dst = gO + (int64_t)j * c + col;
                    *dst = gacc[ct][e] * un + *dst;
                }
            }
        }
    }
};

// Sweep 2.  Workgroup w: entity tiles (128 rows) w, w + grid, ...; every query tile.
template <int KS, int SG, typename LK>
__global__ __launch_bounds__(64 * BS_WAVES, 1) void go_kernel(const unsigned char *__restrict__ qp,
                                                              const unsigned char *__restrict__ vp,
                                                              const unsigned char *__restrict__ qx, int B,
                                                              const float *__restrict__ O, int N, int c, LK lk,
                                                              const float *__restrict__ v_bound, float *__restrict__ gO) {
    GoSweep<KS, SG, LK> pol{vp, qx, B, N, c, ldexpf(1.0f, -14 - rtk_pack_shift(v_bound[0])), lk, gO};
    sweep<float, KS, SG>(pol, qp, B, O, N, c, true, (int)gridDim.x, 1);
}

// the entity ranges of sweep 1: the chip filled once by (query groups x splits)
int splits_of(int64_t batch) {
    const int64_t n_qg = rtk_cdiv(rtk_cdiv(batch, 32), BS_WAVES);
    const int64_t s = RTK_N_CU / (n_qg > 0 ? n_qg : 1);
    return (int)(s < 1 ? 1 : s);
}

// ---- host side -------------------------------------------------------------------------------------------------

// The workspace pieces both losses use (byte offsets; [0, 256): the error word's header).  A loss takes its own partial
// buffers behind them, so those offsets move with max_pos: a call fills what it reads, and nothing in the workspace but
// the error word may be carried from one call (rows) to another (grad).  bounds: max |O|, max |s v|.
struct StreamWs {
    size_t bounds, rows_pos, slab, dvpos, vs, vp, off, ent, owner, dzf, sort, total;
    size_t take(size_t bytes) {
        const size_t p = total;
        total += rtk_align_up(bytes, 256);
        return p;
    }
};
// nct_pad: the column tiles of the slabs and of the images of s v where a sweep pads them (0: nct_of)
StreamWs stream_layout(int64_t batch, int c, int64_t max_pos, int nct_pad = 0) {
    StreamWs L;
    const int nct = nct_pad ? nct_pad : nct_of((c + 15) / 16);
    const size_t B = (size_t)batch, S = (size_t)splits_of(batch), n_mt = (size_t)rtk_cdiv(batch, 32);
    const size_t M = (size_t)(max_pos > 0 ? max_pos : 0);
    L.total = 256;
    L.bounds = L.take(256);
    L.rows_pos = L.take(B * BS_POS_Y * 8);
    L.slab = L.take(S * B * 32 * nct * 4);
    L.dvpos = L.take(B * (size_t)c * 4);
    L.vs = L.take(B * (size_t)c * 4);
    L.vp = L.take(n_mt * (size_t)nct * 4096);
    L.off = L.take((B + 1) * 4);
    L.ent = L.take(M * 4);
    L.owner = L.take(M * 4);
    L.dzf = L.take(M * 4);
    L.sort = L.take(rtk_scatter_bytes((int64_t)M));
    return L;
}

// what both losses require of max_pos and the label smoothing (check_block's `own`), the shapes for which their
// *_workspace_bytes answer, and gO of an empty batch: no term touches any row
int check_pos_eps(const char *fn, int64_t max_pos, float eps) {
    RTK_REQUIRE(max_pos >= 0, RTK_ERR_BAD_ARG, "%s: max_pos = %lld must be >= 0", fn, (long long)max_pos);
    RTK_REQUIRE(eps >= 0.f && eps < 1.f, RTK_ERR_BAD_ARG, "%s: label smoothing %g outside [0, 1)", fn, (double)eps);
    RTK_REQUIRE(max_pos < (1ll << 31) - 1, RTK_ERR_UNSUPPORTED, "%s: dimension too large", fn);
    return RTK_OK;
}
bool stream_shape_ok(int64_t batch, int64_t n_ent, int c, int64_t max_pos) {
    return batch >= 0 && n_ent >= 1 && c >= 1 && c <= 16 * BS_MAX_KS && max_pos >= 0 && max_pos < (1ll << 31) - 1;
}
int zero_go(const char *fn, float *gO, int64_t rows, int c, hipStream_t st) {
    return gO ? rtk_zero_async(fn, gO, (size_t)rows * c * 4, st) : RTK_OK;
}

// What comes before sweep 2, for the link LP of the positives: vs = scale v and its packed images of NCT column tiles,
// the positives' flat lists (dt = 1 - eps) and the ordered scatter, which writes gO in full.
template <typename T, int KS, int SG, typename LP>
int go_prologue(const unsigned char *qp, const float *v, int B, int c, int NCT, const T *O, int N, int col0,
                const int64_t *slot, const int64_t *ptr, const int64_t *obj, int64_t max_pos, float dt, const float *scale,
                float *gO, unsigned char *ws, const StreamWs &L, hipStream_t st, const char *fn) {
    const int n_mt = (int)rtk_cdiv(B, 32);
    uint32_t *err = reinterpret_cast<uint32_t *>(ws);
    float *bounds = reinterpret_cast<float *>(ws + L.bounds), *vs = reinterpret_cast<float *>(ws + L.vs);
    int32_t *off = reinterpret_cast<int32_t *>(ws + L.off), *ent = reinterpret_cast<int32_t *>(ws + L.ent);
    int32_t *owner = reinterpret_cast<int32_t *>(ws + L.owner);
    float *dzf = reinterpret_cast<float *>(ws + L.dzf);
    const int64_t nv = (int64_t)B * c;
    hipLaunchKernelGGL(scale_v_kernel, dim3((unsigned)(rtk_cdiv(nv, 256) < 1024 ? rtk_cdiv(nv, 256) : 1024)), dim3(256), 0, st,
                       v, nv, scale, vs);
    int rc = rtk_absmax_f32(vs, B, c, c, bounds + 1, (void *)st);
    if (rc != RTK_OK) return rc;
    hipLaunchKernelGGL(pack_v_kernel, dim3((unsigned)n_mt), dim3(256), 0, st, vs, B, c, NCT, bounds + 1,
                       reinterpret_cast<_Float16 *>(ws + L.vp));
    // the positives' share: flat lists, then the ordered scatter (which zeroes gO first)
    if (max_pos > 0) {
        hipLaunchKernelGGL(pos_fill_kernel, dim3((unsigned)(rtk_cdiv(max_pos, 256) < 1024 ? rtk_cdiv(max_pos, 256) : 1024)),
                           dim3(256), 0, st, max_pos, (int32_t)N, ent, owner, dzf);
        hipLaunchKernelGGL(pos_offsets_kernel, dim3(1), dim3(256), 0, st, B, slot, ptr, max_pos, off, err);
        hipLaunchKernelGGL((pos_kernel<T, KS, SG, LP>), dim3((unsigned)B), dim3(64 * BS_WAVES), 0, st, qp, B, O, N, col0, c, dt,
                           slot, ptr, obj, (double *)nullptr, (float *)nullptr, (const int32_t *)off, max_pos, ent, owner, dzf);
    }
    return rtk_scatter_flat(fn, ent, owner, dzf, max_pos, N, vs, c, gO, ws + L.sort, st);
}

// Sweep 2 with everything before it, for the links LP (positives) and LK (sweep; qx: what travels with its query
// tiles, LK::QB bytes each): go_prologue, then go_kernel on top of the positives' share.  A static launch sequence.
template <int KS, int SG, typename LP, typename LK>
int launch_go(const unsigned char *qp, const float *v, int B, int c, const float *O, int N, int col0, const int64_t *slot,
              const int64_t *ptr, const int64_t *obj, int64_t max_pos, float dt, const float *scale, LK lk,
              const unsigned char *qx, float *gO, unsigned char *ws, const StreamWs &L, hipStream_t st, const char *fn) {
    const int rc = go_prologue<float, KS, SG, LP>(qp, v, B, c, nct_of(KS), O, N, col0, slot, ptr, obj, max_pos, dt, scale, gO,
                                                  ws, L, st, fn);
    if (rc != RTK_OK) return rc;
    const float *bounds = reinterpret_cast<const float *>(ws + L.bounds);
    // one workgroup per CU: whole entity tiles per slot, no query ranges
    const int n_slots = grid_of(B, N, RTK_N_CU).n_slots;
    return launch_lds<&go_kernel<KS, SG, LK>, GoLds<KS, LK::QB>::TOTAL>(dim3((unsigned)n_slots), dim3(64 * BS_WAVES), st, fn, qp,
                                                                        (const unsigned char *)(ws + L.vp), qx, B, O, N, c, lk,
                                                                        (const float *)(bounds + 1), gO);
}

}  // namespace
