// Shared helpers for the gfx950 kernels of librtucker_hip.so (internal header).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stddef.h>
#include <utility>

#include "rtucker_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define RTK_WAVE 64

// host side ---------------------------------------------------------------
void rtk_set_error(const char *fmt, ...);
#define RTK_REQUIRE(cond, code, ...)            \
    do {                                        \
        if (!(cond)) {                          \
            rtk_set_error(__VA_ARGS__);         \
            return (code);                      \
        }                                       \
    } while (0)

// Kernel timer (rtk_timer_*, rtk_abi.hip): a score-kernel launcher asks whether the calling thread armed a timer; if so
// the launch goes through hipExtLaunchKernelGGL with the timer's two events, which the runtime stamps with the kernel's
// own begin / end times (what a rocprofv3 kernel trace reports), not with the stream's progress around the launch.
bool rtk_take_launch_events(hipEvent_t *start, hipEvent_t *stop);
#define RTK_LAUNCH_SCORE(kernel, grid, block, smem, st, ...)                                                      \
    do {                                                                                                          \
        hipEvent_t ev0_, ev1_;                                                                                    \
        if (rtk_take_launch_events(&ev0_, &ev1_))                                                                 \
            hipExtLaunchKernelGGL(kernel, grid, block, smem, st, ev0_, ev1_, 0, __VA_ARGS__);                     \
        else                                                                                                      \
            hipLaunchKernelGGL(kernel, grid, block, smem, st, __VA_ARGS__);                                       \
    } while (0)

static inline int rtk_check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        rtk_set_error("%s: %s", what, hipGetErrorString(e));
        return RTK_ERR_LAUNCH;
    }
    return RTK_OK;
}

// Kernels that need more than 64 KiB of dynamic LDS must raise hipFuncAttributeMaxDynamicSharedMemorySize,
// and the attribute is kept PER DEVICE: a process that scores on a second GPU has to set it there too.
// `done` is a per-instantiation bitmask of device ordinals already configured (atomic: callers may be
// multi-threaded); devices >= 64 set the attribute on every launch (idempotent).
#include <atomic>
static inline int rtk_ensure_dynamic_lds(const void *kernel, int bytes, std::atomic<unsigned long long> &done,
                                         const char *what) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) {
        const unsigned long long bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
        if (bit && (done.load(std::memory_order_acquire) & bit)) return RTK_OK;
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) {
            if (bit) done.fetch_or(bit, std::memory_order_release);
            return RTK_OK;
        }
    }
    rtk_set_error("%s: cannot reserve %d bytes of dynamic LDS: %s", what, bytes, hipGetErrorString(e));
    return RTK_ERR_LAUNCH;
}

static inline int rtk_zero_async(const char *fn, void *p, size_t bytes, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e == hipSuccess) return RTK_OK;
    rtk_set_error("%s: memset: %s", fn, hipGetErrorString(e));
    return RTK_ERR_LAUNCH;
}

static inline size_t rtk_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int64_t rtk_cdiv(int64_t x, int64_t y) { return (x + y - 1) / y; }

// Runtime k-step count -> template argument: returns f(std::integral_constant<int, ks>{}) for 1 <= ks <= KMAX (f is
// instantiated for every one of them), else RTK_ERR_UNSUPPORTED.  The packed query planes were written for exactly
// `ks` k-steps (tile stride), so a score kernel's instantiation must match exactly.
template <typename F, int... I>
static inline int rtk_dispatch_ksteps_(int ks, const char *what, F &f, std::integer_sequence<int, I...>) {
    int rc = RTK_ERR_UNSUPPORTED;
    if (!((ks == I + 1 && ((rc = f(std::integral_constant<int, I + 1>{})), true)) || ...))
        rtk_set_error("%s: unsupported k-step count %d", what, ks);
    return rc;
}
template <int KMAX, typename F>
static inline int rtk_dispatch_ksteps(int ks, const char *what, F &&f) {
    return rtk_dispatch_ksteps_(ks, what, f, std::make_integer_sequence<int, KMAX>{});
}

// Runtime (16-byte chunks per lane of a row, vector path) -> template arguments: f(integral_constant<int, nch>, bool
// constant) for nch = 1 .. NMAX (NMAX = 2 or 4), instantiated for every pair.  Another nch launches nothing and is an
// error: a row is never cut short.
template <int NMAX, typename F>
static inline int rtk_dispatch_chunks(const char *fn, int nch, bool vec, F &&f) {
    auto by_vec = [&](auto nc) { vec ? f(nc, std::true_type{}) : f(nc, std::false_type{}); };
    RTK_REQUIRE(nch >= 1 && nch <= NMAX, RTK_ERR_UNSUPPORTED, "%s: %d chunks per row, at most %d", fn, nch, NMAX);
    if (nch == 1) by_vec(std::integral_constant<int, 1>{});
    else if (nch == 2) by_vec(std::integral_constant<int, 2>{});
    else if constexpr (NMAX == 4) {
        if (nch == 3) by_vec(std::integral_constant<int, 3>{});
        else by_vec(std::integral_constant<int, 4>{});
    }
    return rtk_check_launch(fn);
}

// Workspace layout (all offsets 256-B aligned), see rtk_abi.hip::ws_layout
struct RtkWorkspace {
    uint32_t *flags;      // [0] error word, [1] number of distinct relations (n_u)
    int32_t *slot_of_rel; // n_rel : relation id -> table slot (or -1)
    int32_t *rel_list;    // min(n_rel, B) : slot -> relation id
    float *tables;        // n_u_max * b * c : M_u = G x_0 R[u]
    float *v;             // B * c fp32 query vectors
    void *q_packed;       // packed query planes
    void *core_t;         // bf16, relation rank > 32: core transposed to [(b,c)][a]
    void *r_packed;       // bf16, relation rank > 32: packed planes of the batch's relation rows
    int32_t *grp_cnt;     // 2 * n_u_max : queries per table slot; scatter cursor
    int32_t *grp_order;   // B : query ids sorted by table slot
    int32_t *grp_work;    // 4 * (B / 4 + n_u_max) : contract work items (slot, first, count, -)
    int64_t *grp_qinfo;   // 2 * B : per position in slot order (subject id, query id | slot << 32)
    size_t total;
};

// device side -------------------------------------------------------------
#ifdef __HIPCC__
// Operand element types: float, or bf16 carried as its raw 16 bits (torch.bfloat16 storage).
typedef unsigned short rtk_bf16;
__device__ __forceinline__ float rtk_to_f32(float x) { return x; }
__device__ __forceinline__ float rtk_to_f32(rtk_bf16 x) { return __builtin_bit_cast(float, (unsigned)x << 16); }
// round-to-nearest-even fp32 -> bf16 bits (NaN stays NaN: plain cast semantics of v_cvt_pk_bf16_f32)
__device__ __forceinline__ rtk_bf16 rtk_f32_to_bf16(float x) {
    return __builtin_bit_cast(rtk_bf16, (__bf16)x);
}
// 4 consecutive elements -> f32x4 (p must be 16-B aligned for float, 8-B aligned for bf16)
__device__ __forceinline__ f32x4 rtk_load4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ f32x4 rtk_load4(const rtk_bf16 *p) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 w = *reinterpret_cast<const u32x2 *>(p);
    f32x4 r;
    r[0] = __builtin_bit_cast(float, w[0] << 16);
    r[1] = __builtin_bit_cast(float, w[0] & 0xffff0000u);
    r[2] = __builtin_bit_cast(float, w[1] << 16);
    r[3] = __builtin_bit_cast(float, w[1] & 0xffff0000u);
    return r;
}
// Element q of 16 bytes of a row held as four words (through a scalar: a bit_cast straight from the vector element
// returned element 0 for every q)
__device__ __forceinline__ float rtk_bits_elem(const u32x4 &w, int q, float) {
    const unsigned x = w[q];
    return __builtin_bit_cast(float, x);
}
__device__ __forceinline__ float rtk_bits_elem(const u32x4 &w, int q, rtk_bf16) {
    const unsigned x = w[q >> 1];
    return __builtin_bit_cast(float, (q & 1) ? (x & 0xffff0000u) : (x << 16));
}
// 16 bytes of row `row` at element j0 (4 fp32 / 8 bf16), zero past c.  VEC: the row is 16-B aligned and c % VW == 0.
template <typename T, bool VEC>
__device__ __forceinline__ u32x4 rtk_load_piece(const T *__restrict__ row, int j0, int c) {
    if constexpr (VEC) {
        if (j0 < c) return *reinterpret_cast<const u32x4 *>(row + j0);
        return u32x4{0u, 0u, 0u, 0u};
    }
    u32x4 w{0u, 0u, 0u, 0u};
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = j0 + q < c ? __builtin_bit_cast(unsigned, (float)row[j0 + q]) : 0u;
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const unsigned h = j0 + q < c ? (unsigned)row[j0 + q] : 0u;
            w[q >> 1] |= (q & 1) ? (h << 16) : h;
        }
    }
    return w;
}
template <typename T> __host__ __device__ constexpr int rtk_vec4_align() { return sizeof(T) == 4 ? 16 : 8; }
// Correctly behaving fp32 logistic: 1/(1+exp(-x)) with ocml expf (<= 1 ulp) and an
// IEEE division, the same formula torch's CPU kernel evaluates; saturates to
// exactly 1.0f for x >~ 16.64 like the reference.
__device__ __forceinline__ float rtk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// ln x on v_log_f32 (log2, 1 ulp), clamped at -100 like torch's BCE.  v_log_f32 reads a subnormal x as 0, and the exact
// logistic (an IEEE division) does return subnormal probabilities (ln p between -87.3 and -103.3), as may any score
// matrix a caller hands in: those are scaled by 2^32 first.  A normal x gives the bits of the plain form.  The one
// copy for every kernel that sums BCE terms of STORED or exactly computed probabilities (rtk_rank.hip,
// rtk_score_rank_kernel.h, rtk_bce.hip), so that their bits stay equal.
__device__ __forceinline__ float rtk_clog(float x) {
    const bool sub = x < 1.17549435e-38f;
    const float l2 = __builtin_amdgcn_logf(sub ? x * 4294967296.0f : x) - (sub ? 32.0f : 0.0f);
    return fmaxf(l2 * 0.6931471805599453f, -100.0f);
}
#endif
