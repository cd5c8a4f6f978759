// The candidate order of the top-k selection as unsigned keys (internal header): rtk_topk.hip selects on them,
// rtk_score_topk.hip takes its tile maxima in the same order, so a NaN wins its tile exactly as it wins the select.
#pragma once
#include "rtk_common.h"

namespace {

__device__ __forceinline__ uint32_t sel_key(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;   // every NaN -> +NaN, above +inf
    if (u == 0x80000000u) u = 0u;                             // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t sel_key(rtk_bf16 x) {
    uint32_t u = x;
    if ((u & 0x7fffu) > 0x7f80u) u = 0x7fc0u;
    if (u == 0x8000u) u = 0u;
    return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}
// key 0 lies below every real key (-inf maps to 0x007fffff / 0x007f): the padding key
__device__ __forceinline__ float sel_value(uint32_t k, float) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float sel_value(uint32_t k, rtk_bf16) {
    return __uint_as_float(((k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu)) << 16);
}

}  // namespace
