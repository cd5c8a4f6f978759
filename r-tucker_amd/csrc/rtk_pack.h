// "Packed query planes": the layout stage 1 writes and the split-fp16 / bf16 score
// kernels stream through LDS.  One block per tile of 32 queries:
//
//   [ 32 x float : per-row unscale factor 2^-sh_d            ]   RTK_PACK_HDR = 128 B
//   [ plane 0 (hi) : ksteps x 2 (k-half) x 32 (row) x 8 x 16-bit ]   1024*ksteps B
//   [ plane 1 (lo) : same                                       ]   (fp32 path only)
//
// i.e. exactly the A-operand fragment order of v_mfma_f32_32x32x16_{f16,bf16}
// (lane l holds A[row = l & 31][k = 16*ks + 8*(l >> 5) + j], j = 0..7 -- 16 contiguous
// bytes), so a wave's fragment read is one linear, conflict-free 1-KiB ds_read_b128.
// Element v[d,k] of the fp32 path is stored as  hi = fp16(x), lo = fp16(x - hi) with
// x = v[d,k] * 2^sh_d and sh_d chosen so the row maximum lands in [2^14, 2^15): both
// halves stay inside fp16's normal range, hi + lo carries ~22 significand bits.
// The only device code that writes this layout is rtk_pack_store_row_* at the end of this file.
#pragma once
#include <stdint.h>
#include <math.h>

#define RTK_PACK_HDR 128

#if defined(__HIPCC__)
#define RTK_HD __host__ __device__ __forceinline__
#else
#define RTK_HD static inline
#endif

RTK_HD int64_t rtk_pack_tile_bytes(int ksteps, int planes) { return RTK_PACK_HDR + (int64_t)planes * ksteps * 1024; }

// index (in 16-bit elements, within a plane) of element k of row `row`
RTK_HD int rtk_pack_offset(int ksteps, int k, int row) {
    (void)ksteps;
    return (((k >> 4) * 2 + ((k >> 3) & 1)) * 32 + row) * 8 + (k & 7);
}

// power-of-two shift that brings a row maximum `mx` (>= 0) into [2^14, 2^15)
RTK_HD int rtk_pack_shift(float mx) {
    if (!(mx > 0.f) || !(mx < INFINITY)) return 0;
    int e;
    (void)frexpf(mx, &e);        // mx = m * 2^e, m in [0.5, 1)  ->  floor(log2 mx) = e - 1
    int sh = 14 - (e - 1);
    return sh > 100 ? 100 : (sh < -100 ? -100 : sh);
}

#if defined(__HIPCC__)
#include "rtk_common.h"   // rtk_bf16, rtk_f32_to_bf16: the bf16 writer stores the bits the kernels' loads widen

// Row d of the packed planes at `packed`, stored by thread t of a workgroup of nthreads (k = t, t + nthreads, ...);
// columns c <= k < 16 * ksteps are zeros.
// fp32 path: header 2^-sh, then x = v * 2^sh as fp16 hi / lo planes.  row: the c values (LDS or global); mx: the row's
// largest magnitude, already reduced over the workgroup.
__device__ __forceinline__ void rtk_pack_store_row_f32(unsigned char *packed, int64_t d, int ksteps, const float *row, int c,
                                                       float mx, int t, int nthreads) {
    const int sh = rtk_pack_shift(mx);
    const float up = ldexpf(1.0f, sh);
    unsigned char *tile = packed + (d >> 5) * rtk_pack_tile_bytes(ksteps, 2);
    const int r = (int)(d & 31);
    if (t == 0) reinterpret_cast<float *>(tile)[r] = ldexpf(1.0f, -sh);
    _Float16 *planes = reinterpret_cast<_Float16 *>(tile + RTK_PACK_HDR);
    for (int k = t; k < ksteps * 16; k += nthreads) {
        const float x = (k < c) ? row[k] * up : 0.f;
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        const int off = rtk_pack_offset(ksteps, k, r);
        planes[off] = hi;
        planes[off + ksteps * 512] = lo;  // plane 1 follows plane 0 (ksteps*2*32*8 halves)
    }
}

// bf16 path: header 1.0f (bf16 has fp32's range: no scaling), then one plane.  bits(k) gives the bf16 bits of column
// k for every k < 16 * ksteps, the zero columns included.
template <typename F>
__device__ __forceinline__ void rtk_pack_store_row_bf16(unsigned char *packed, int64_t d, int ksteps, int t, int nthreads, F bits) {
    unsigned char *tile = packed + (d >> 5) * rtk_pack_tile_bytes(ksteps, 1);
    const int r = (int)(d & 31);
    if (t == 0) reinterpret_cast<float *>(tile)[r] = 1.0f;
    rtk_bf16 *plane = reinterpret_cast<rtk_bf16 *>(tile + RTK_PACK_HDR);
    for (int k = t; k < ksteps * 16; k += nthreads) plane[rtk_pack_offset(ksteps, k, r)] = bits(k);
}
// ... from c fp32 values, rounded to nearest even
__device__ __forceinline__ void rtk_pack_store_row_bf16(unsigned char *packed, int64_t d, int ksteps, const float *row, int c,
                                                        int t, int nthreads) {
    rtk_pack_store_row_bf16(packed, d, ksteps, t, nthreads, [=](int k) { return rtk_f32_to_bf16((k < c) ? row[k] : 0.f); });
}
#endif
