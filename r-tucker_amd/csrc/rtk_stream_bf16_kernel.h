// The two sweeps of the matrix-free training losses on bf16 entity rows, c <= 512 (rtk_bce_stream_bf16.hip; internal
// header beside rtk_stream_kernel.h, whose pos_kernel, images of s v, flat lists and workspace pieces serve both).
//
// A wave cannot keep a whole row of the dv / gO accumulator at c = 512 (16 column tiles of 16 registers on top of the
// operand fragments), so the second tile product of both sweeps is CUT ALONG THE OUTPUT COLUMNS: the 32-column tiles
// are dealt to nch_of(KS) chunks of cct_of(KS) <= 4 tiles (128 columns), the chunk is blockIdx.y, and every chunk
// computes the score tile again.  The chunks of a sweep write disjoint columns, so nothing is added across them.
//
//   rows_sweep_bf16   sweep 1, the structure of rows_sweep: query on the lane, the entity tile copied once per
//                     workgroup into LDS as the chain's operand (bf16 as it is: one plane, no per-row scaling) and, for
//                     dv, the chunk's columns as ONE fp16 plane scaled by the power of two of max |O| (a bf16 value
//                     has 8 significant bits: fp16 holds it exactly down to the fp16 subnormals).  The k-steps are
//                     summed as Frag<rtk_bf16, KS>::chain_with sums them (two chains at KS <= 16, one above), so a
//                     probability has the bits of the bf16 score, rank and top-k kernels.
//   GoSweepBf16       sweep 2, a policy of sweep<rtk_bf16, KS, SG>: the tile of x against the chunk's tiles of the
//                     image of s v (pack_v_kernel's two f16 planes, padded to nctp_of(KS) tiles).
//
// x is split as in the fp32 form (2^14, f16 hi/lo): two MFMAs per k-step against O, three against s v.
#pragma once
#include "rtk_stream_kernel.h"

namespace {

constexpr int BSB_MAX_KS = SW_MAX_KS_BF16;     // c <= 512
constexpr int BSB_MAX_CT = 4;                  // column tiles of a chunk: 64 accumulator registers

__host__ __device__ constexpr int nch_of(int ks) { return (nct_of(ks) + BSB_MAX_CT - 1) / BSB_MAX_CT; }       // chunks
__host__ __device__ constexpr int cct_of(int ks) { return (nct_of(ks) + nch_of(ks) - 1) / nch_of(ks); }       // tiles per chunk
__host__ __device__ constexpr int nctp_of(int ks) { return nch_of(ks) * cct_of(ks); }                         // tiles, padded

// acc[ct] += X * T for one plane `timg` of a transposed image
template <int CT>
__device__ __forceinline__ void tile_product_1(const f16x8 (&xh)[2], const f16x8 (&xl)[2], const f16x8 *__restrict__ timg,
                                               int lane, f32x16 (&acc)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f16x8 b = timg[(ct * 2 + t) * 64 + lane];
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[t], b, acc[ct], 0, 0, 0);
            acc[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl[t], b, acc[ct], 0, 0, 0);
        }
}

template <int KS>
struct RowsLdsBf16 {
    static constexpr int CT = cct_of(KS);
    static constexpr int A1 = 0;                       // [KS][64] x 16 B: the tile's rows as the chain's operand
    static constexpr int T2 = KS * 1024;               // one plane of the transposed image of the chunk's columns
    static constexpr int TOTAL = T2 + CT * 2048;
};

// max |x| of n bf16 values (n % 8 == 0, x 16-byte aligned) as a float in out[0], which the caller zeroed: the maximum of
// the 15 magnitude bits is the magnitude of the maximum
__global__ __launch_bounds__(256) void absmax_bf16_kernel(const rtk_bf16 *__restrict__ x, int64_t n, float *__restrict__ out) {
    unsigned m = 0;
    const u32x4 *p = reinterpret_cast<const u32x4 *>(x);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n / 8; i += (int64_t)gridDim.x * 256) {
        const u32x4 w = p[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned a = w[q] & 0x7fff7fffu;
            m = max(m, max(a >> 16, a & 0xffffu));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(reinterpret_cast<unsigned *>(out), m << 16);
}

// Sweep 1, the skeleton.  Workgroup (qg, sp) of chunk blockIdx.y: query tiles 4 qg .. 4 qg + 3 (one per wave), entity
// tiles of split sp, output columns [32 CT chunk, 32 CT (chunk + 1)) of dv.  The policy:
//
//   begin(d, on)                 before the sweep; d is the lane's query, `on` whether its tile exists
//   tile(acc, tile, h, N, x)     the accumulators of one entity tile (element e: entity row acc_row(e, h) of the tile,
//                                the lane's query); fills x, the tile of the logit gradient
//   finish(sp, d, h, B)          after the sweep: the policy's partial results of split sp
//
// O: the vector row path (c % 8 == 0, 16-byte aligned), a 16-byte piece is wholly inside or outside a row.
template <int KS, int SG, bool DV, typename P>
__device__ __forceinline__ void rows_sweep_bf16(P &pol, const unsigned char *__restrict__ qp, int B,
                                                const rtk_bf16 *__restrict__ O, int N, int c,
                                                const float *__restrict__ o_bound, int n_splits, float *__restrict__ slab) {
    typedef RowsLdsBf16<KS> L;
    constexpr int CT = L::CT, CP = 32 * nctp_of(KS);
    constexpr int NP = (2 * KS + 7) / 8;               // 16-byte pieces of a row per staging thread
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const int qg = (int)blockIdx.x / n_splits, sp = (int)blockIdx.x % n_splits;
    const int col_lo = (int)blockIdx.y * (32 * CT);                 // the chunk's first column
    const int n_mt = (B + 31) >> 5, n_t = (N + 31) >> 5;
    const int mt = qg * BS_WAVES + wave;
    const bool active = mt < n_mt;                                  // (wave-uniform)
    const int tb = (int)((int64_t)n_t * sp / n_splits), te = (int)((int64_t)n_t * (sp + 1) / n_splits);

    bf16x8 Q[KS];
    if (active) {
        load_a<rtk_bf16, KS>(qp, mt, r, h, Q, Q);
    } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Q[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    pol.begin(mt * 32 + r, active);
    f32x16 dacc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dacc[ct] = zero16();
    const float up2 = DV ? ldexpf(1.0f, rtk_pack_shift(o_bound[0])) : 1.0f;

    // staging: 8 consecutive threads take one row, thread `part` the pieces part, part + 8, ...
    const int srw = t >> 3, part = t & 7;
    u32x4 stg[NP];
    auto stage_load = [&](int tile) {
        const rtk_bf16 *row = O + (int64_t)min(tile * 32 + srw, N - 1) * c;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int k0 = 8 * (part + 8 * i);
            stg[i] = (k0 + 8 <= c) ? *reinterpret_cast<const u32x4 *>(row + k0) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto stage_store = [&]() {
        _Float16 *t2 = reinterpret_cast<_Float16 *>(lds + L::T2);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int f = part + 8 * i;                             // piece f: k = 8 f .. 8 f + 7, k-step f / 2, half f % 2
            if (f >= 2 * KS) continue;
            *reinterpret_cast<u32x4 *>(lds + L::A1 + ((f >> 1) * 64 + (f & 1) * 32 + srw) * 16) = stg[i];
            const int cl = 8 * f - col_lo;                          // (columns past 16 KS stay unwritten: they feed output columns >= c, never stored)
            if (DV && cl >= 0 && cl < 32 * CT) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    t2[timg_index(srw, cl + q)] = (_Float16)(rtk_bits_elem(stg[i], q, rtk_bf16{}) * up2);
            }
        }
    };

    if (tb < te) stage_load(tb);
    for (int tile = tb; tile < te; ++tile) {
        stage_store();
        __syncthreads();
        if (tile + 1 < te) stage_load(tile + 1);
        if (active) {
            const bf16x8 *la = reinterpret_cast<const bf16x8 *>(lds + L::A1);
            f32x16 acc = zero16(), acc2 = zero16();
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {                       // Frag<rtk_bf16, KS>::chain_with with the roles swapped
                const bf16x8 e = la[ks * 64 + lane];
                if (KS <= 16 && (ks & 1)) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(e, Q[ks], acc2, 0, 0, 0);
                else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(e, Q[ks], acc, 0, 0, 0);
            }
            if (KS <= 16) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = acc[e] + acc2[e];
            }
            float x[16];
            pol.tile(acc, tile, h, N, x);
            if (DV) {
                f16x8 xh[2], xl[2];
                split_x(x, xh, xl);
                tile_product_1<CT>(xh, xl, reinterpret_cast<const f16x8 *>(lds + L::T2), lane, dacc);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    pol.finish(sp, mt * 32 + r, h, B);
    if (DV) {
        // element e of dacc[ct]: query row acc_row(e, h) of the tile, column col_lo + 32 ct + r
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int dq = mt * 32 + acc_row(e, h);
                if (dq < B) slab[((int64_t)sp * B + dq) * CP + col_lo + ct * 32 + r] = dacc[ct][e];
            }
    }
}

// LDS of sweep 2: the packed query tile (header + one plane) and the chunk's tiles of the image of s v behind it
template <int KS>
struct GoLdsBf16 {
    static constexpr int TILE = (int)tile_bytes<rtk_bf16, KS>();
    static constexpr int IMG = cct_of(KS) * 4096;                  // two planes of CT column tiles
    static constexpr int TOTAL = 2 * (TILE + IMG);
};

// What go_bf16_kernel does with the sweep: GoSweep's part on the chunk's columns.  vp holds, per query tile, the two
// planes of nctp_of(KS) column tiles (pack_v_kernel); a chunk's tiles are contiguous within a plane.  The link LK
// turns an accumulated value into x: x<SG>(f, acc, srow, q, valid).
template <int KS, int SG, typename LK>
struct GoSweepBf16 {
    static constexpr int CT = cct_of(KS), NCTP = nctp_of(KS);
    static constexpr int TILE = GoLdsBf16<KS>::TILE, IMG = GoLdsBf16<KS>::IMG, EXTRA = IMG;
    static constexpr int NLV = IMG / 16 / (64 * BS_WAVES);          // 16-byte pieces of the chunk's image per thread: CT
    static_assert(IMG % (16 * 64 * BS_WAVES) == 0, "the image of s v is staged without a bound: whole pieces per thread");
    const unsigned char *__restrict__ vp;
    int B, N, c, chunk;
    float un;
    LK lk;
    float *__restrict__ gO;
    u32x4 vstg[NLV];
    f32x16 gacc[CT];

    __device__ __forceinline__ void load_extra(SweepLane ln, int mt) {
        const u32x4 *sv = reinterpret_cast<const u32x4 *>(vp + (int64_t)mt * NCTP * 4096) + chunk * CT * 128;
#pragma unroll
        for (int i = 0; i < NLV; ++i) {
            const int ix = i * 64 * BS_WAVES + ln.t, plane = ix >= CT * 128;       // pieces [0, 128 CT): plane 0
            vstg[i] = sv[plane * NCTP * 128 + ix - plane * CT * 128];
        }
    }
    __device__ __forceinline__ void store_extra(SweepLane ln, int extra) const {
        u32x4 *dst = reinterpret_cast<u32x4 *>(sweep_lds + extra);
#pragma unroll
        for (int i = 0; i < NLV; ++i) dst[i * 64 * BS_WAVES + ln.t] = vstg[i];
    }
    __device__ __forceinline__ void begin_tile() {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) gacc[ct] = zero16();
    }
    // element e: query row acc_row(e, h) of the tile, entity r of the wave
    __device__ __forceinline__ void score(SweepLane ln, const Frag<rtk_bf16, KS> &f, const f32x16 &acc,
                                          const unsigned char *buf, int, int, bool, int mt) {
        float x[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = lk.template x<SG>(f, acc[e], 1.0f, e & 3, mt * 32 + acc_row(e, ln.h) < B);
        f16x8 xh[2], xl[2];
        split_x(x, xh, xl);
        tile_product<CT>(xh, xl, reinterpret_cast<const f16x8 *>(buf + TILE), ln.lane, gacc);
    }
    __device__ __forceinline__ void publish(SweepLane, int, int, int, int, int, bool) const {}
    // element e of gacc[ct]: entity row acc_row(e, h) of the wave, column 32 (CT chunk + ct) + r; on top of the
    // positives' share that the ordered scatter wrote
    __device__ __forceinline__ void end_tile(SweepLane ln, int tile) const {
        const int j0 = tile * SW_TILE + ln.wave * 32;                // the wave's first row
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int col = (chunk * CT + ct) * 32 + ln.r;
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

// Sweep 2.  Workgroup (w, chunk): entity tiles (128 rows) w, w + grid, ...; every query tile; the chunk's columns.
template <int KS, int SG, typename LK>
__global__ __launch_bounds__(64 * BS_WAVES, 1) void go_bf16_kernel(const unsigned char *__restrict__ qp,
                                                                   const unsigned char *__restrict__ vp, int B,
                                                                   const rtk_bf16 *__restrict__ O, int N, int c, LK lk,
                                                                   const float *__restrict__ v_bound,
                                                                   float *__restrict__ gO) {
    GoSweepBf16<KS, SG, LK> pol{vp, B, N, c, (int)blockIdx.y, ldexpf(1.0f, -14 - rtk_pack_shift(v_bound[0])), lk, gO};
    sweep<rtk_bf16, KS, SG>(pol, qp, B, O, N, c, true, (int)gridDim.x, 1);
}

}  // namespace
