// Launcher of the wave-specialised persistent split-fp16 score kernel (rtk_score_ws_kernel.h).
#include "rtk_score_select.h"
#include "rtk_score_ws_kernel.h"

namespace {

template <int KS, int SG>
int launch_v(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld, hipStream_t st) {
    constexpr bool OV = true;   // the plan guarantees c % 4 == 0 and a 16-byte-aligned O
    const size_t smem = rtk_ws::lds_bytes<KS>(c);
    static std::atomic<unsigned long long> lds_ok{0};
    const int rc = rtk_ensure_dynamic_lds(reinterpret_cast<const void *>(&rtk_ws::score_ws_kernel<KS, SG, OV>),
                                          160 * 1024, lds_ok, "score_ws_kernel");
    if (rc != RTK_OK) return rc;
    // one resident workgroup per CU; the kernel cuts the (entity tile x query tile) space evenly
    const int64_t units = rtk_cdiv(N, 128) * rtk_cdiv(B, 32);
    const unsigned grid = (unsigned)(units < RTK_N_CU ? units : RTK_N_CU);
    const int xcd_remap = 2;   // XCD-aware schedule of the remainder tiles only (the kernel also has 0 off, 1 both phases)
    const int nts = (ld * 4) % 128 == 0 && (reinterpret_cast<uintptr_t>(out) & 127) == 0;   // nontemporal score stores
    RTK_LAUNCH_SCORE((rtk_ws::score_ws_kernel<KS, SG, OV>), dim3(grid), dim3(512), smem, st, qp, B, O, N, c, out, ld,
                     xcd_remap, nts);
    return RTK_OK;
}

}  // namespace

int rtk_score_ws_launch(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld, int sg,
                        hipStream_t st) {
    return rtk_dispatch_ksteps<RTK_CG_MAX_KS>((c + 15) / 16, "rtk_score_packed_f32", [&](auto K) {
        if (sg == 0) return launch_v<K.value, 0>(qp, B, O, N, c, out, ld, st);
        if (sg == 1) return launch_v<K.value, 1>(qp, B, O, N, c, out, ld, st);
        return launch_v<K.value, 2>(qp, B, O, N, c, out, ld, st);
    });
}
