// Operand fragments of the matrix-free ranking and loss kernels (rtk_score_rank.hip, rtk_bce_stream.hip; internal
// header): the B fragments of one entity row, their conversion, the MFMA chain against the packed query planes and the
// logistic.  Both files take every probability from here, so a (query row, entity row, c) triple has the same bits in
// the entity-stationary kernels (count_kernel, the loss sweeps) and in the per-query passes (target_kernel,
// filter_kernel).
#pragma once
#include "rtk_common.h"
#include "rtk_pack.h"

namespace {

// (the clamped logarithm of the BCE terms is rtk_clog, rtk_common.h)

// Operand form of one element type: B fragments of one entity row per lane pair (r, h), A fragments of the packed
// planes, and the logistic of the accumulated value.
template <typename T, int KS>
struct Frag;

// fp32 operands: split fp16, two planes (rtk_pack.h), per-row power-of-two scaling.
template <int KS>
struct Frag<float, KS> {
    static constexpr int PLANES = 2;
    f16x8 Bh[KS], Bl[KS];
    float kcol;                                   // column factor: 2^-sh of the O row (times -log2 e, fast logistic)
    f32x4 raw[2 * KS];
    // raw row j, lane (r, h): k = 16 ks + 8 h + q (B-operand map of 32x32x16); out-of-row floats read as 0
    __device__ __forceinline__ void load(const float *__restrict__ O, int64_t j, int c, int h, bool) {
        const float *row = O + j * c;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = 16 * ks + 8 * h;
            raw[2 * ks] = (k + 4 <= c) ? *reinterpret_cast<const f32x4 *>(row + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            raw[2 * ks + 1] = (k + 8 <= c) ? *reinterpret_cast<const f32x4 *>(row + k + 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    // the ws kernel's conversion (m_role): row maximum over both lanes of the row, shift, hi = fp16(y), lo = fp16(y - hi)
    template <int SG>
    __device__ __forceinline__ void convert() {
        float mx = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int q = 0; q < 4; ++q) mx = fmaxf(mx, fmaxf(fabsf(raw[2 * ks][q]), fabsf(raw[2 * ks + 1][q])));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const int sh = rtk_pack_shift(mx);
        const float up = ldexpf(1.0f, sh);
        const float us_o = ldexpf(1.0f, -sh);
        kcol = SG == 2 ? us_o * -1.4426950408889634f : us_o;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float y0 = raw[2 * ks][q] * up, y1 = raw[2 * ks + 1][q] * up;
                const _Float16 h0 = (_Float16)y0, h1 = (_Float16)y1;
                Bh[ks][q] = h0;
                Bh[ks][4 + q] = h1;
                Bl[ks][q] = (_Float16)(y0 - (float)h0);
                Bl[ks][4 + q] = (_Float16)(y1 - (float)h1);
            }
        }
    }
    // one chain: per k-step hi*hi, hi*lo, lo*hi (the ws kernel's order); a(plane, ks) supplies the A fragment
    template <typename FA>
    __device__ __forceinline__ f32x16 chain_with(FA a) const {
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 acc;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 ah = a(0, ks), al = a(1, ks);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, Bh[ks], ks == 0 ? zero : acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, Bl[ks], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, Bh[ks], acc, 0, 0, 0);
        }
        return acc;
    }
    __device__ __forceinline__ f32x16 chain(const f16x8 (&Ah)[KS], const f16x8 (&Al)[KS]) const {
        return chain_with([&](int plane, int ks) { return plane ? Al[ks] : Ah[ks]; });
    }
    // probability of an accumulated value with row factor `srow` (the packed header's 2^-sh_d)
    template <int SG>
    __device__ __forceinline__ float prob(float acc, float srow) const {
        const float s = srow * kcol;
        if (SG == 2) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc * s));
        return rtk_sigmoid(acc * s);
    }
};

// bf16 operands: one plane, no scaling; the k-steps in two chains (even, odd) added at KS <= 16, one chain above
// (score_bf16_kernel: both forms of an instantiation give these bits).
template <int KS>
struct Frag<rtk_bf16, KS> {
    static constexpr int PLANES = 1;
    bf16x8 Bf[KS];
    bf16x8 nxt[KS];
    // vec: c % 8 == 0 and O 16-byte aligned (a fragment is wholly inside or outside the row); the values are the same
    __device__ __forceinline__ void load(const rtk_bf16 *__restrict__ O, int64_t j, int c, int h, bool vec) {
        const rtk_bf16 *row = O + j * c;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = 16 * ks + 8 * h;
            bf16x8 x = {0, 0, 0, 0, 0, 0, 0, 0};
            if (vec) {
                if (k + 8 <= c) x = *reinterpret_cast<const bf16x8 *>(row + k);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (k + q < c) x[q] = (short)row[k + q];
            }
            nxt[ks] = x;
        }
    }
    template <int SG>
    __device__ __forceinline__ void convert() {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Bf[ks] = nxt[ks];
    }
    // a(plane, ks) supplies the A fragment (one plane)
    template <typename FA>
    __device__ __forceinline__ f32x16 chain_with(FA a) const {
        f32x16 acc, acc2;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = acc2[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 af = a(0, ks);
            if (KS <= 16 && (ks & 1)) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, Bf[ks], acc2, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, Bf[ks], acc, 0, 0, 0);
        }
        if (KS <= 16) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = acc[e] + acc2[e];
        }
        return acc;
    }
    __device__ __forceinline__ f32x16 chain(const bf16x8 (&A)[KS], const bf16x8 (&)[KS]) const {
        return chain_with([&](int, int ks) { return A[ks]; });
    }
    template <int SG>
    __device__ __forceinline__ float prob(float z, float) const {
        if (SG == 2) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(z * -1.4426950408889634f));
        return 1.0f / (1.0f + expf(-z));
    }
};

template <typename T> struct AFrag { typedef f16x8 type; };
template <> struct AFrag<rtk_bf16> { typedef bf16x8 type; };

template <typename T, int KS>
__host__ __device__ constexpr int64_t tile_bytes() { return RTK_PACK_HDR + (int64_t)Frag<T, KS>::PLANES * KS * 1024; }

// A fragments of row `row` of packed tile `mt` (lane (i, h) reads row `row`'s k-half h): the same 16 bytes the stored
// kernels read from LDS when row == lane & 31
template <typename T, int KS>
__device__ __forceinline__ void load_a(const unsigned char *__restrict__ qp, int mt, int row, int h,
                                       typename AFrag<T>::type (&A0)[KS], typename AFrag<T>::type (&A1)[KS]) {
    typedef typename AFrag<T>::type AT;
    const AT *p0 = reinterpret_cast<const AT *>(qp + mt * tile_bytes<T, KS>() + RTK_PACK_HDR);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        A0[ks] = p0[ks * 64 + h * 32 + row];
        if (Frag<T, KS>::PLANES == 2) A1[ks] = p0[(KS + ks) * 64 + h * 32 + row];
    }
}

}  // namespace
