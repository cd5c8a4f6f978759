// Launcher of the column-group split-fp16 score kernel (rtk_score_cg_kernel.h).
// Compiled three times (build.sh), once per logistic variant RTK_CG_SG = 0 (logits), 1 (exact), 2 (fast):
// 13 k-step counts x 4 M-wave roles x 2 sweeps each.  Which kernel runs, and this one's set schedule, is decided in
// rtk_score_select.h.
#include "rtk_score_cg_kernel.h"
#include "rtk_score_select.h"

#ifndef RTK_CG_SG
#error "compile with -DRTK_CG_SG=0|1|2"
#endif
static_assert(rtk_cg::NG == RTK_CG_GROUPS_PER_SET, "rtk_score_plan_f32 schedules the kernel's sets");

namespace {

template <int KS, int SG>
int launch_v(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld, int W, int U,
             hipStream_t st) {
    const size_t smem = rtk_cg::lds_bytes<KS>(c);
    static std::atomic<unsigned long long> lds_ok{0};
    const int rc = rtk_ensure_dynamic_lds(reinterpret_cast<const void *>(&rtk_cg::score_cg_kernel<KS, SG>), 160 * 1024,
                                          lds_ok, "score_cg_kernel");
    if (rc != RTK_OK) return rc;
    const int nts = (ld * 4) % 128 == 0 && (reinterpret_cast<uintptr_t>(out) & 127) == 0;   // nontemporal score stores
    const int tune = 0;   // wave priorities off (the kernel's A/B parameter)
    RTK_LAUNCH_SCORE((rtk_cg::score_cg_kernel<KS, SG>), dim3(W), dim3(512), smem, st, qp, B, O, N, c, out, ld, U,
                     (int)(rtk_cdiv(N, 32) / U), (int)(rtk_cdiv(N, 32) % U), nts, tune);
    return RTK_OK;
}

}  // namespace

template <int SG>
int rtk_score_cg_launch(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld,
                        const RtkScorePlan &plan, hipStream_t st) {
    return rtk_dispatch_ksteps<RTK_CG_MAX_KS>((c + 15) / 16, "rtk_score_packed_f32", [&](auto K) {
        return launch_v<K.value, SG>(qp, B, O, N, c, out, ld, plan.W, plan.U, st);
    });
}
template int rtk_score_cg_launch<RTK_CG_SG>(const unsigned char *, int, const float *, int, int, float *, int64_t,
                                            const RtkScorePlan &, hipStream_t);

#if RTK_CG_SG == 2 && defined(RTK_CG_STAMPS)
// tools/ablate: copy out (dst != NULL) or clear (clear != 0) the timeline of the fast-logistic instantiation
extern "C" int rtk_cg_timeline(unsigned long long *dst, int n, int clear) {
    static unsigned long long zeros[256 * 2 * 64];
    if (clear && hipMemcpyToSymbol(HIP_SYMBOL(rtk_cg::g_cg_tl), zeros, sizeof(zeros)) != hipSuccess) return -1;
    if (dst && hipMemcpyFromSymbol(dst, HIP_SYMBOL(rtk_cg::g_cg_tl), (size_t)n * 8) != hipSuccess) return -2;
    return 0;
}
#endif
