// The BCE link functions the matrix-free BCE kernels share (rtk_bce_stream.hip: fp32 operands, rtk_bce_stream_bf16.hip:
// bf16 operands; internal header): what a probability adds as a negative, what a CSR entry adds on top of it, and x of
// sweep 2.  F is the operand form, Frag<float, KS> or Frag<rtk_bf16, KS>.
#pragma once
#include "rtk_stream_kernel.h"

namespace {

// x of one probability and its BCE term as a negative
__device__ __forceinline__ float x_of(float p, float t0, bool valid) {
    return (valid && p != 1.0f && p != 0.0f) ? p - t0 : 0.0f;
}

// the positives' link: the correction -(1 - eps) (ln p - ln(1 - p)) and dz = -(1 - eps), 0 where p is saturated
struct BcePos {
    static __device__ __forceinline__ float coef(float dt, int64_t) { return dt; }
    template <int SG, typename F>
    static __device__ __forceinline__ void term(const F &f, float acc, float srow, float dt, float &lacc, float &dz) {
        const float p = f.template prob<SG>(acc, srow);
        lacc += dt * (rtk_clog(p) - rtk_clog(1.0f - p));
        dz = (p == 1.0f || p == 0.0f) ? 0.f : -dt;
    }
};

// sweep 2's link: nothing travels with the query tile
struct BceGo {
    static constexpr int QB = 0;
    float t0;
    __device__ __forceinline__ void rows4(const unsigned char *, int) {}
    template <int SG, typename F>
    __device__ __forceinline__ float x(const F &f, float acc, float srow, int, bool valid) const {
        return x_of(f.template prob<SG>(acc, srow), t0, valid);
    }
};

}  // namespace
