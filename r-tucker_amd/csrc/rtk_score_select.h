// Which fp32 split-fp16 score kernel rtk_score_packed_f32 launches, and the launchers it picks from (internal header).
// rtk_score_plan_f32 is the one place the rule lives: the launch, rtk_score_kernel_f32 and
// rtk_score_fifth_group_columns_f32 (what Python and the tests ask) all take it from here.
#pragma once
#include "rtk_common.h"

constexpr int RTK_N_CU = 256;         // workgroups of the persistent kernels: one per MI355X CU
constexpr int RTK_CG_MAX_KS = 13;     // cg and ws kernels: c <= 208
constexpr int RTK_CG_GROUPS_PER_SET = 5;   // rtk_cg::NG

struct RtkScorePlan {
    unsigned kernel;   // RTK_SCORE_KERNEL_CG / _WS / _V3
    int W, U;          // cg: workgroups and sets (U / W sets per workgroup, one after the other)
};

// The cg set schedule: G = ceil(N/32) column groups in U = W * P sets of <= 5 consecutive groups, P sets per workgroup:
// ceil(G / 5) sets when that fills the chip, else min(G, 256) sets of 1-5 groups (all CUs busy; up to 1024 groups no
// set has a fifth group and every score has the ws kernel's bits).  Without a hint cg runs for one set per workgroup
// (P = 1) with at least two groups in it: 18 432 <= N <= 40 960 on 256 CUs (tools/ab_cg_shapes.py, c = 200, B = 512,
// back to back: N = 20 000 22.3 us against 24.5 for the ws kernel, 26 000 25.0 / 28.8, 32 000 25.9 / 32.7,
// 36 000 31-33 / 40, 40 943 (WN18RR: 1280 groups = 5 per CU exactly) 32-34 / 36-41; at 14 951 the two tie, at 16 384
// (the ws kernel's tiles divide evenly) it is 10 % ahead, from 46 000 on -- two passes here, each with its own exposed
// prologue -- the ws kernel's tile schedule is 1-10 % ahead).  Otherwise the persistent wave-specialised kernel (ws);
// the two-workgroups-per-CU kernel (v3) has the scalar paths (c % 4 != 0 or unaligned O) and c > 208.  A hint picks
// the kernel on every shape it covers.  (The two-tiles-per-barrier variant "ws2" was measured slower, 53.9 vs 48.5 us
// at the WN18RR shape, and lives in tools/ablate/ only.)
static inline RtkScorePlan rtk_score_plan_f32(int64_t n_local, int c, bool o_vec, unsigned flags) {
    const unsigned hint = flags & RTK_SCORE_KERNEL_MASK;
    if (hint == RTK_SCORE_KERNEL_V3 || !o_vec || (c + 15) / 16 > RTK_CG_MAX_KS) return {RTK_SCORE_KERNEL_V3, 0, 0};
    const int64_t G = rtk_cdiv(n_local, 32);
    int64_t sets = rtk_cdiv(G, RTK_CG_GROUPS_PER_SET);
    if (sets < RTK_N_CU) sets = G < RTK_N_CU ? G : RTK_N_CU;
    const int64_t W = sets < RTK_N_CU ? sets : RTK_N_CU;
    const int64_t P = rtk_cdiv(sets, W);
    const bool cg = hint == RTK_SCORE_KERNEL_CG || (hint == 0 && P == 1 && G >= 576);
    if (cg && P * W <= (1 << 30)) return {RTK_SCORE_KERNEL_CG, (int)W, (int)(P * W)};
    return {RTK_SCORE_KERNEL_WS, 0, 0};
}

// c <= 512: two fp16 planes of B fragments must fit the register file next to the pipeline state
static inline bool rtk_split_ksteps_supported(int c) { return c >= 1 && c <= 512; }

// Launchers (rtk_score_ws.hip, rtk_score_cg.hip): launch what they are given, return an rtk_status.
// sg: 0 logits, 1 exact logistic, 2 fast logistic.  Both need c % 4 == 0 and a 16-byte-aligned O.
int rtk_score_ws_launch(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld, int sg,
                        hipStream_t st);
// One object per logistic variant (build.sh compiles rtk_score_cg.hip with -DRTK_CG_SG=0|1|2).
template <int SG>
int rtk_score_cg_launch(const unsigned char *qp, int B, const float *O, int N, int c, float *out, int64_t ld,
                        const RtkScorePlan &plan, hipStream_t st);
