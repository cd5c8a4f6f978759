// The split-fp16 score kernel (included by rtk_score_split.hip and by the ablation
// build tools/ablate/rtk_score_ablate.hip).  Design notes: rtk_score_split.hip.
#pragma once
#include "rtk_common.h"
#include "rtk_pack.h"

namespace rtk_split {

// tools/ablate only (ABL bit 6): per-block phase stamps (s_memrealtime, 100 MHz)
__device__ unsigned long long g_stamps[4096 * 4];
__device__ unsigned long long g_istamps[4096 * 8];   // ABL bit 7: s_memtime stamps inside iteration 3

// SIGMOID: 0 = raw logits, 1 = ocml expf + IEEE divide (torch-CPU formula, ~25 VALU),
//          2 = 1 / (1 + 2^(-z log2 e)) on v_exp_f32 + v_rcp_f32 (4 VALU, 1 ulp each)
// LOSS (training forward; reference train.py:79,136 + Dataset.py:51-52): instead of the probability p
// the epilogue writes x = p - t0 (+0 where p is saturated to exactly 1.0f, -0 where it is 0.0f: the reference's
// autograd returns a zero logit gradient there) -- d BCE / d logit of an entry whose label-smoothed target is the negatives'
// t0 = eps / N, up to the factor g / (B N) that the backward applies to the small operands -- and adds the entry's
// BCE term -(t0 ln p + (1 - t0) ln(1 - p)) (logs on v_log_f32, clamped at -100 like torch) to a per-lane sum that
// leaves the kernel as ONE double per workgroup in partials[blockIdx.x].  The few positives are patched afterwards
// (rtk_bce.hip: bce_patch_pos_kernel).  The B x N matrix is written once and never re-read in the forward.
// split_clog is the plain form, without rtk_clog's rescaling of subnormals (rtk_common.h), on purpose: its argument is
// a probability from the fast logistic, and v_rcp_f32 returns no subnormal -- over z = -89.5 .. -87 in steps of 2^-10
// the kernel's p goes from 1.1762094e-38 (z = -87.33594) straight to 0 -- while 1.0f - p is 0 or
// at least 2^-24.  The epilogue lives in the MFMA shadow; it is not given VALU work that cannot change a bit.
__device__ __forceinline__ float split_clog(float x) { return fmaxf(__builtin_amdgcn_logf(x) * 0.6931471805599453f, -100.0f); }

template <int KS, int SIGMOID, int MINW, unsigned ABL = 0, bool LOSS = false>
__global__ __launch_bounds__(256, MINW) void score_split_kernel(
    const unsigned char *__restrict__ q_packed, int B, const float *__restrict__ O, int N, int c,
    float *__restrict__ out, int64_t ld_out, bool o_vec, float t0 = 0.f, double *__restrict__ partials = nullptr) {
    // ABL != 0 only in tools/ablate (compile-time ablations): bit0 skip staging, bit1 skip MFMA,
    // bit2 skip stores, bit3 skip the query sweep (prologue only), bit4 skip the O conversion,
    // bit5 skip the barriers
    auto off = [](unsigned bit) { return (ABL & bit) != 0; };
    constexpr int TILE_BYTES = RTK_PACK_HDR + 2 * KS * 1024;
    constexpr int CHUNKS = TILE_BYTES / 16;
    constexpr int NLD = (CHUNKS + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];  // 2 * TILE_BYTES

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int n_mt = (B + 31) / 32;
    // linearised (entity tile, query tile) space split evenly over the grid: perfect
    // balance, at most one extra O-tile conversion per block
    const int64_t U = (int64_t)((N + 127) / 128) * n_mt;
    int64_t lin = U * blockIdx.x / gridDim.x;
    const int64_t lin_end = U * (blockIdx.x + 1) / gridDim.x;

    int stamp_n = 0;
    double loss_sum = 0.0;         // LOSS: this lane's share of the batch's BCE terms (as +sum of y ln p + (1-y) ln(1-p))
    float loss_tile = 0.f;
    int ep_rows = 0;
    if (off(64) && t == 0) g_stamps[blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memrealtime();
    while (lin < lin_end) {
        const int ntile = (int)(lin / n_mt), mt0 = (int)(lin % n_mt);
        const int cnt = (int)min((int64_t)(n_mt - mt0), lin_end - lin);
        lin += cnt;
        const int j = ntile * 128 + wave * 32 + r;  // entity (row of O, column of out)

        // ---- this lane's slice of O row j -> scaled hi/lo fp16 B fragments ----
        // lane (r, h) holds k = 16*ks + 8*h + q, q < 8  (B-operand map of 32x32x16).  One
        // round of loads straight into registers (all 2*KS float4 in flight together: a single
        // exposed memory latency, no LDS phase, no barrier), then row max -> power-of-two
        // scale -> hi/lo split in place.  Every byte of O is requested exactly once.
        const float *orow = O + (int64_t)min(j, N - 1) * c;
        float raw[KS][8];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = 16 * ks + 8 * h;
            if (off(16)) {
#pragma unroll
                for (int q = 0; q < 8; ++q) raw[ks][q] = (float)(lane + q + ks);
            } else if (o_vec) {  // c % 4 == 0: each float4 is wholly inside or wholly outside the row
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
                if (k + 4 <= c) a = *reinterpret_cast<const f32x4 *>(orow + k);
                if (k + 8 <= c) b = *reinterpret_cast<const f32x4 *>(orow + k + 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    raw[ks][q] = a[q];
                    raw[ks][4 + q] = b[q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) raw[ks][q] = (k + q < c) ? orow[k + q] : 0.f;
            }
        }
        float mx = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int q = 0; q < 8; ++q) mx = fmaxf(mx, fabsf(raw[ks][q]));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const int sh = rtk_pack_shift(mx);
        const float up = ldexpf(1.0f, sh);
        const float us_o = ldexpf(1.0f, -sh);
        f16x8 Bh[KS], Bl[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float y = raw[ks][q] * up;
                const _Float16 hi = (_Float16)y;
                Bh[ks][q] = hi;
                Bl[ks][q] = (_Float16)(y - (float)hi);
            }
        }
        if (off(64) && t == 0 && stamp_n == 0) { g_stamps[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime(); stamp_n = 1; }
        if (off(8)) {  // prologue only: keep the fragments alive
            float keep = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) keep += (float)Bh[ks][0] + (float)Bl[ks][7];
            if (keep == 12345.678f) out[0] = keep;
            continue;
        }

        // ---- sweep `cnt` query tiles, software pipelined ----
        //   iteration i:  global loads of tile i+1 in flight  |  MFMAs of tile i  |
        //                 logistic + stores of tile i-1       |  ds_write tile i+1 ; barrier
        u32x4 stg[NLD];
        auto stage_load = [&](int mt) {
            const u32x4 *src = reinterpret_cast<const u32x4 *>(q_packed + (int64_t)mt * TILE_BYTES);
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int ch = i * 256 + t;
                if (!off(1) && (i + 1 < NLD || ch < CHUNKS)) stg[i] = src[ch];
            }
        };
        auto stage_store = [&](int buf) {
            u32x4 *dst = reinterpret_cast<u32x4 *>(lds + buf * TILE_BYTES);
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int ch = i * 256 + t;
                if (!off(1) && (i + 1 < NLD || ch < CHUNKS)) dst[ch] = stg[i];
            }
        };
        // Stores go through a buffer descriptor rebased per query tile: rows past B fall
        // outside num_records and lanes past N carry a poisoned offset, so the hardware
        // drops them -- the epilogue is branch-free and the scheduler can place it in the
        // shadow of the next tile's MFMA chain.
        const unsigned voff = (j < N) ? (unsigned)((4 * h * ld_out + j) * 4) : 0x80000000u;
        __amdgpu_buffer_rsrc_t ers;  // descriptor of the tile whose epilogue is running
        unsigned ep_off = voff;      // running byte offset of the next store (kept out of LICM's reach)
        const unsigned ld4 = (unsigned)(ld_out * 4);
        auto epilogue_begin = [&](int mt, bool live) {
            const int rows = live ? min(32, B - mt * 32) : 0;
            ep_rows = rows;
            ers = __builtin_amdgcn_make_buffer_rsrc(out + (int64_t)max(mt, 0) * 32 * ld_out, 0,
                                                    (unsigned)(rows * ld_out * 4), 0x00020000);
            ep_off = voff;
            asm volatile("" : "+v"(ep_off));   // one live register instead of 16 hoisted offsets
        };
        // The epilogue of one tile is cut into 32 pieces (16 accumulator elements x
        // {exponential half, reciprocal half + store}) that the k-loop drops into the gaps
        // between its dependent MFMAs: a 32x32x16 MFMA occupies the matrix pipe for 32 cycles
        // but the wave's issue port for 8, so ~6 independent VALU instructions issue for free.
        float ep_d = 1.f, ep_p = 1.f;
        auto piece = [&](const f32x16 &z, int pc) {
            const int e = pc >> 1;
            if ((pc & 1) == 0) {
                if (SIGMOID == 2) {
                    ep_d = __builtin_amdgcn_exp2f(z[e] * -1.4426950408889634f);   // 2^t = inf for very negative z: p = 0
                } else if (SIGMOID == 1) {
                    ep_d = 1.0f + expf(-z[e]);
                } else {
                    ep_p = z[e];
                }
            } else {
                float pv = ep_p;
                if (SIGMOID == 2) pv = __builtin_amdgcn_rcpf(1.0f + ep_d);   // v_exp_f32 / v_rcp_f32 are 1-ulp
                if (SIGMOID == 1) pv = 1.0f / ep_d;
                const int row = (e & 3) + 8 * (e >> 2);  // + 4*h inside voff
                if (LOSS) {
                    const float term = t0 * split_clog(pv) + (1.0f - t0) * split_clog(1.0f - pv);
                    if (j < N && row + 4 * h < ep_rows) loss_tile += term;
                    // (the sign of the zero tells the patch kernel which; a score that merely EQUALS t0 -- p = eps / N is an
                    // ordinary fp32 value, e.g. 2.4e-6 at WN18RR: a positive with logit -12.9 -- must not read as saturated:
                    // it is stored as the smallest denormal, 1.4e-45 away from its exact logit gradient of zero)
                    const float xv = pv - t0;
                    pv = (pv == 1.0f) ? 0.0f : ((pv == 0.0f) ? -0.0f : (xv == 0.0f ? __builtin_bit_cast(float, 1u) : xv));
                }
                if (off(4)) {
                    if (pv == 12345.678f) out[0] = pv;
                } else {
                    (void)row;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, pv), ers, ep_off, 0, 0);
                    ep_off += ((e & 3) == 3) ? 5u * ld4 : ld4;   // rows 0,1,2,3,8,9,10,11,16,...
                }
            }
        };

        stage_load(mt0);
        stage_store(0);
        __syncthreads();
        f32x16 prev;
#pragma unroll
        for (int e = 0; e < 16; ++e) prev[e] = 0.f;
        for (int i = 0; i < cnt; ++i) {
            const int cur = i & 1;
            const bool stamp_it = off(128) && i == 3 && lane == 0;
            if (stamp_it) g_istamps[(blockIdx.x * 4 + wave) * 8 + 0] = __builtin_amdgcn_s_memtime();
            if (i + 1 < cnt) stage_load(mt0 + i + 1);
            if (stamp_it) g_istamps[(blockIdx.x * 4 + wave) * 8 + 1] = __builtin_amdgcn_s_memtime();
            const unsigned char *tile = lds + cur * TILE_BYTES;
            const f16x8 *lh = reinterpret_cast<const f16x8 *>(tile + RTK_PACK_HDR);
            const f16x8 *ll = lh + KS * 64;
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            epilogue_begin(mt0 + i - 1, i > 0);
            constexpr int GAPS = 3 * KS;  // one gap after every MFMA
            f16x8 ah = lh[lane], al = ll[lane];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                f16x8 nh = ah, nl = al;
                if (ks + 1 < KS) {  // A fragments one k-step ahead
                    nh = lh[(ks + 1) * 64 + lane];
                    nl = ll[(ks + 1) * 64 + lane];
                }
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const int g = 3 * ks + m;
                    if (off(2)) {
                        acc[g & 15] += (float)ah[m] * (float)Bh[ks][m] + (float)al[m] * (float)Bl[ks][m];
                    } else {
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(m == 2 ? al : ah, m == 1 ? Bl[ks] : Bh[ks], acc, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // keep the gap's pieces BEHIND their MFMA (see rtk_score_ws_kernel.h)
#pragma unroll
                    for (int pc = g * 32 / GAPS; pc < (g + 1) * 32 / GAPS; ++pc) piece(prev, pc);
                    __builtin_amdgcn_sched_barrier(0);
                }
                ah = nh;
                al = nl;
            }
            if (stamp_it) g_istamps[(blockIdx.x * 4 + wave) * 8 + 2] = __builtin_amdgcn_s_memtime();
            // unscale while this tile's row factors are still in LDS:
            // C/D map  column = lane & 31 (entity), row = (e & 3) + 8*(e >> 2) + 4*h
            const float *lscale = reinterpret_cast<const float *>(tile);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 sv = *reinterpret_cast<const f32x4 *>(lscale + 8 * g + 4 * h);
#pragma unroll
                for (int q = 0; q < 4; ++q) prev[4 * g + q] = acc[4 * g + q] * sv[q] * us_o;
            }
            if (LOSS) {
                loss_sum += (double)loss_tile;
                loss_tile = 0.f;
            }
            stage_store(cur ^ 1);  // unconditional: a stale tile in the spare buffer is never read
            if (stamp_it) g_istamps[(blockIdx.x * 4 + wave) * 8 + 3] = __builtin_amdgcn_s_memtime();
            if (!off(32)) __syncthreads();
            if (stamp_it) g_istamps[(blockIdx.x * 4 + wave) * 8 + 4] = __builtin_amdgcn_s_memtime();
        }
        epilogue_begin(mt0 + cnt - 1, true);
#pragma unroll
        for (int pc = 0; pc < 32; ++pc) piece(prev, pc);
        if (LOSS) {
            loss_sum += (double)loss_tile;
            loss_tile = 0.f;
        }
    }
    if (LOSS) {     // one double per workgroup, lanes and waves added in a fixed order (deterministic)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) loss_sum += __shfl_xor(loss_sum, o);
        __syncthreads();
        double *red = reinterpret_cast<double *>(lds);
        if (lane == 0) red[wave] = loss_sum;
        __syncthreads();
        if (t == 0) partials[blockIdx.x] = -(red[0] + red[1] + red[2] + red[3]);
    }
    if (off(64) && t == 0) g_stamps[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace rtk_split
