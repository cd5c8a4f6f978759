// What the matrix-free kernels on entity blocks share (rtk_score_rank.hip, rtk_score_topk.hip, rtk_bce_stream.hip;
// internal header):
//
//   Frag<T, KS>      the B fragments of one entity row, their conversion, the MFMA chain against the packed query planes
//                    and the logistic.  All three files take every probability from here, so a (query row, entity row,
//                    c) triple has the same bits in the entity-stationary sweeps, in the per-query passes and in
//                    rows_kernel (which calls row_scale and logistic on its own operand layout).
//   QueryRow<T, KS>  one query against a few entity rows by one wave: the per-query passes (target_kernel,
//                    filter_kernel, patch_kernel / gather_kernel, pos_kernel).
//   reduce16         the halving butterfly over the 32 entity lanes (sum or maximum), red_row its lane-to-row map.
//   sweep            the entity-stationary loop of count_kernel, tmax_kernel and go_kernel: what differs between them
//                    is a policy object (what travels with a query tile, the epilogues, the hooks around an entity tile).
//   host side        SweepGrid / grid_of, vec_rows, check_block, dispatch, launch_lds.
#pragma once
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_select.h"

// the dynamic LDS of a sweep kernel: the two staging buffers, then what the kernel's policy keeps behind them
extern __shared__ __attribute__((aligned(16))) unsigned char sweep_lds[];

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
    // the scaling of a row with largest magnitude `mx`: y = x * up = x * 2^sh, and the column factor 2^-sh (times -log2 e,
    // fast logistic) that prob puts back
    template <int SG>
    static __device__ __forceinline__ void row_scale(float mx, float &up, float &kc) {
        const int sh = rtk_pack_shift(mx);
        up = ldexpf(1.0f, sh);
        const float us_o = ldexpf(1.0f, -sh);
        kc = SG == 2 ? us_o * -1.4426950408889634f : us_o;
    }
    // the logistic of an accumulated value with row factor `srow` and column factor `kc`
    template <int SG>
    static __device__ __forceinline__ float logistic(float acc, float srow, float kc) {
        const float s = srow * kc;
        if (SG == 2) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(acc * s));
        return rtk_sigmoid(acc * s);
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
        float up;
        row_scale<SG>(mx, up, kcol);
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
    __device__ __forceinline__ float prob(float acc, float srow) const { return logistic<SG>(acc, srow, kcol); }
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
    static __device__ __forceinline__ float prob(float z, float) {
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

// One query against entity rows, by one wave: the A fragments of query d in all 32 rows of the tile and the query's row
// factor, so that element 0 of lane r (h == 0) is the probability of the entity row that lane r loaded.
template <typename T, int KS>
struct QueryRow {
    typename AFrag<T>::type A0[KS], A1[KS];
    float srow;
    __device__ __forceinline__ void load(const unsigned char *__restrict__ qp, int d, int h) {
        const int mt = d >> 5, row = d & 31;
        load_a<T, KS>(qp, mt, row, h, A0, A1);
        srow = Frag<T, KS>::PLANES == 2 ? reinterpret_cast<const float *>(qp + mt * tile_bytes<T, KS>())[row] : 1.0f;
    }
    // p(d, O[j]) for the row j of this lane's column (lanes r and r + 32 pass the same j); f: the caller's fragment
    // registers (one Frag serves all the calls of a wave)
    template <int SG>
    __device__ __forceinline__ float score(Frag<T, KS> &f, const T *__restrict__ O, int64_t j, int c, int h,
                                           bool vec) const {
        f.load(O, j, c, h, vec);
        f.template convert<SG>();
        const f32x16 acc = f.chain(A0, A1);
        return f.template prob<SG>(acc[0], srow);
    }
};

// Row of a 32 x 32 accumulator tile that element e of a lane of half h holds (the column is the lane's r).
__device__ __forceinline__ int acc_row(int e, int h) { return 8 * (e >> 2) + 4 * h + (e & 3); }

// v[0 .. 15] combined over the 32 lanes of a half wave.  Each step trades half of the live values with lane ^ O_ and
// keeps the other half, so 8 + 4 + 2 + 1 exchanges and one last full one do the work of 16 x 5.  Afterwards lane r
// holds the result of element red_elem(r), row red_row(r, h) of the tile; the order of the combinations is fixed.
struct RedSum {
    template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return a + b; }
};
struct RedMax {
    template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return max(a, b); }
};
template <int N, int O_, typename V, typename Op>
__device__ __forceinline__ void reduce_step(V (&v)[16], int r, Op op) {
    const bool up = (r & O_) != 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const V send = up ? v[i] : v[i + N];
        const V keep = up ? v[i + N] : v[i];
        v[i] = op(keep, (V)__shfl_xor(send, O_));
    }
}
template <typename V, typename Op>
__device__ __forceinline__ V reduce16(V (&v)[16], int r, Op op) {
    reduce_step<8, 16>(v, r, op);
    reduce_step<4, 8>(v, r, op);
    reduce_step<2, 4>(v, r, op);
    reduce_step<1, 2>(v, r, op);
    return op(v[0], (V)__shfl_xor(v[0], 1));
}
__device__ __forceinline__ int red_elem(int r) { return (r >> 1) & 15; }   // bits 4..1 of r, most significant first
__device__ __forceinline__ int red_row(int r, int h) { return acc_row(red_elem(r), h); }

constexpr int SW_WAVES = 4;                    // waves per workgroup of a sweep: 128 entity rows per tile
constexpr int SW_TILE = 32 * SW_WAVES;
constexpr int SW_SLOTS = 2 * RTK_N_CU;         // resident workgroups of the two-per-CU sweeps
constexpr int SW_MAX_KS_F32 = RTK_CG_MAX_KS;   // the ws kernel's range: c <= 208
constexpr int SW_MAX_KS_BF16 = 32;             // score_bf16_kernel's range: c <= 512

// A thread's place in a sweep's workgroup: wave, and lane (r, h) of the MFMA tile
struct SweepLane {
    int t, lane, wave, r, h;
};

// The row of O that row jl of the block reads: jl itself, unless the policy maps it (an optional hook, row_of(jl))
template <typename P>
__device__ __forceinline__ auto sweep_row(const P &pol, int jl, int) -> decltype(pol.row_of(jl)) { return pol.row_of(jl); }
template <typename P>
__device__ __forceinline__ int sweep_row(const P &, int jl, long) { return jl; }

// The entity-stationary sweep.  Workgroup (slot, qs) of n_slots x qsplit takes the entity tiles slot, slot + n_slots,
// ... of the block and the query tiles of range qs.  Each wave converts its 32 rows into B fragments ONCE per entity
// tile, keeps them in registers and sweeps the query tiles, whose packed planes the workgroup stages through two LDS
// buffers of tile_bytes + P::EXTRA bytes at the start of sweep_lds (what lies behind them is the policy's).  While a tile
// is scored the next one is on its way from memory in registers; after the last query tile the first one follows, for
// the next entity tile.  The policy P supplies
//
//   EXTRA                  bytes staged behind each query tile
//   load_extra(ln, mt)     fetch them for query tile mt into the policy's registers ...
//   store_extra(ln, at)    ... and write them to sweep_lds + at
//   begin_tile()           before the query loop of an entity tile
//   score(ln, f, acc, buf, cur, jl, valid, mt)
//                          the 32 x 32 accumulators of query tile mt (staged at buf, parity cur) against the wave's
//                          rows (this lane: row jl of the block, `valid` when inside it); before the barrier that
//                          ends the query tile
//   publish(ln, cur, i, mt, slot, tile, first)
//                          after that barrier; i is the tile's place in the range, `first` says that this is the
//                          workgroup's first entity tile
//   end_tile(ln, tile)     after the query loop
//   row_of(jl)             optional: the row of O behind row jl of the block (default: jl; rtk_pair.hip pads its rows)
template <typename T, int KS, int SG, typename P>
__device__ __forceinline__ void sweep(P &pol, const unsigned char *__restrict__ qp, int B, const T *__restrict__ O,
                                      int n_local, int c, bool vec, int n_slots, int qsplit) {
    typedef typename AFrag<T>::type AT;
    constexpr int TILE = (int)tile_bytes<T, KS>(), BUF = TILE + P::EXTRA;
    constexpr int NT = 64 * SW_WAVES;
    constexpr int CHUNKS = TILE / 16;
    constexpr int NLD = (CHUNKS + NT - 1) / NT;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
    const SweepLane ln = {t, lane, wave, r, h};
    const int slot = (int)blockIdx.x / qsplit, qs = (int)blockIdx.x % qsplit;
    const int n_mt = (B + 31) >> 5, n_tiles = (n_local + SW_TILE - 1) / SW_TILE;
    const int mt0 = (int)((int64_t)n_mt * qs / qsplit), nq = (int)((int64_t)n_mt * (qs + 1) / qsplit) - mt0;
    if (nq <= 0 || slot >= n_tiles) return;                       // (never with the host's grid)

    u32x4 stg[NLD];
    auto stage_load = [&](int mt) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(qp + (int64_t)mt * TILE);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ch = i * NT + t;
            if (i + 1 < NLD || ch < CHUNKS) stg[i] = src[ch];
        }
        pol.load_extra(ln, mt);
    };
    auto stage_store = [&](int buf) {
        u32x4 *dst = reinterpret_cast<u32x4 *>(sweep_lds + buf * BUF);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int ch = i * NT + t;
            if (i + 1 < NLD || ch < CHUNKS) dst[ch] = stg[i];
        }
        pol.store_extra(ln, buf * BUF + TILE);
    };

    stage_load(mt0);
    int it = 0;                                                    // tiles staged so far: buffer parity
    for (int tile = slot; tile < n_tiles; tile += n_slots) {
        const int jl = tile * SW_TILE + wave * 32 + r;             // this lane's row of the block
        const bool valid = jl < n_local;
        Frag<T, KS> f;
        f.load(O, sweep_row(pol, min(jl, n_local - 1), 0), c, h, vec);
        f.template convert<SG>();
        pol.begin_tile();
        if (tile == slot) {
            stage_store(0);
            __syncthreads();
        }
        for (int i = 0; i < nq; ++i, ++it) {
            const int cur = it & 1;
            const bool more = i + 1 < nq || tile + n_slots < n_tiles;
            if (more) stage_load(i + 1 < nq ? mt0 + i + 1 : mt0);
            const unsigned char *buf = sweep_lds + cur * BUF;
            const AT *la = reinterpret_cast<const AT *>(buf + RTK_PACK_HDR);
            const f32x16 acc = f.chain_with([&](int plane, int ks) { return la[(plane * KS + ks) * 64 + lane]; });
            pol.score(ln, f, acc, buf, cur, jl, valid, mt0 + i);
            if (more) stage_store(cur ^ 1);
            __syncthreads();
            pol.publish(ln, cur, i, mt0 + i, slot, tile, tile == slot);
        }
        pol.end_tile(ln, tile);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------

// workgroup slots and query ranges of a sweep: whole entity tiles per slot; with fewer tiles than slots the query
// tiles are cut into ranges (each range converts the tile's rows again) until the slots are used
struct SweepGrid {
    int n_slots, qsplit;
};
inline SweepGrid grid_of(int64_t batch, int64_t n_local, int slots) {
    const int64_t n_tiles = rtk_cdiv(n_local, SW_TILE), n_mt = rtk_cdiv(batch, 32);
    SweepGrid g;
    g.n_slots = (int)(n_tiles < slots ? n_tiles : slots);
    int64_t q = slots / (g.n_slots > 0 ? g.n_slots : 1);
    if (q > n_mt) q = n_mt;
    g.qsplit = (int)(q < 1 ? 1 : q);
    return g;
}

// whether O's rows can be read 16 bytes at a time (bf16: a fragment is then wholly inside or outside a row)
template <typename T>
bool vec_rows(const T *O, int c) { return sizeof(T) == 4 || (c % 8 == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0); }

// The checks every entry point on a block [col0, col0 + n_local) of O shares.  `operands`: whether the call's own
// pointers are all there; `own()`: the refusals of the call's own arguments (k, max_pos, ...), tested where the callers
// had them, after the bad arguments and before the unsupported ones, so that a call with several faults keeps its
// return code; `n_ent_limit`: the call's bound on n_ent; `what`: what the call takes on probabilities (nullptr: an entry
// on logits, which has no flags -- `flags` is not looked at); `need()`: the workspace bytes of the call (asked once the
// shape is known to be sound).
template <typename T, typename FO, typename F>
int check_block(const char *fn, bool operands, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0, int64_t n_ent,
                FO own, int64_t n_ent_limit, unsigned flags, const char *what, const void *workspace, size_t ws_bytes, F need) {
    RTK_REQUIRE(operands && O && workspace, RTK_ERR_BAD_ARG, "%s: null operand", fn);
    RTK_REQUIRE(batch >= 0, RTK_ERR_BAD_ARG, "%s: batch = %lld must be >= 0", fn, (long long)batch);
    RTK_REQUIRE(n_ent >= 1, RTK_ERR_BAD_ARG, "%s: n_ent = %lld must be >= 1", fn, (long long)n_ent);
    RTK_REQUIRE(col0 >= 0 && n_local >= 1 && n_local <= n_ent && col0 <= n_ent - n_local, RTK_ERR_BAD_ARG,
                "%s: block col0 = %lld, n_local = %lld is not a non-empty part of [0, n_ent = %lld)", fn, (long long)col0,
                (long long)n_local, (long long)n_ent);
    RTK_REQUIRE(c >= 1, RTK_ERR_BAD_ARG, "%s: object rank c = %d must be >= 1", fn, c);
    const int rc = own();
    if (rc != RTK_OK) return rc;
    RTK_REQUIRE(batch < (1ll << 31) - 32 && n_ent < n_ent_limit, RTK_ERR_UNSUPPORTED, "%s: dimension too large", fn);
    if (what) {
        RTK_REQUIRE(flags & RTK_SCORE_SIGMOID, RTK_ERR_UNSUPPORTED,
                    "%s: %s taken on probabilities: flags need RTK_SCORE_SIGMOID (raw logits are not covered)", fn, what);
        RTK_REQUIRE((flags & ~(RTK_SCORE_SIGMOID | RTK_SCORE_SIGMOID_FAST)) == 0, RTK_ERR_BAD_ARG, "%s: unknown flags 0x%x",
                    fn, flags);
    }
    if (sizeof(T) == 4) {
        RTK_REQUIRE(c <= 16 * SW_MAX_KS_F32, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d (the ws kernel's range)", fn, c,
                    16 * SW_MAX_KS_F32);
        RTK_REQUIRE(c % 4 == 0 && (reinterpret_cast<uintptr_t>(O) & 15) == 0, RTK_ERR_UNSUPPORTED,
                    "%s: fp32 needs c %% 4 == 0 and a 16-byte-aligned O (c = %d)", fn, c);
    } else {
        RTK_REQUIRE(c <= 16 * SW_MAX_KS_BF16, RTK_ERR_UNSUPPORTED, "%s: c = %d above %d", fn, c, 16 * SW_MAX_KS_BF16);
    }
    const size_t bytes = need();
    RTK_REQUIRE(ws_bytes >= bytes, RTK_ERR_BAD_ARG, "%s: workspace of %zu bytes given, %zu needed", fn, ws_bytes, bytes);
    RTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, RTK_ERR_BAD_ARG, "%s: workspace must be 256-byte aligned",
                fn);
    return RTK_OK;
}

// f(K, SG) instantiated for the k-steps of c and the logistic the flags select, then the launch check
template <typename T, typename F>
int dispatch(const char *fn, int c, unsigned flags, F f) {
    const bool fast = (flags & RTK_SCORE_SIGMOID_FAST) != 0;
    const int rc = rtk_dispatch_ksteps<sizeof(T) == 4 ? SW_MAX_KS_F32 : SW_MAX_KS_BF16>((c + 15) / 16, fn, [&](auto K) {
        return fast ? f(K, std::integral_constant<int, 2>{}) : f(K, std::integral_constant<int, 1>{});
    });
    return rc != RTK_OK ? rc : rtk_check_launch(fn);
}

// A timed launch of `Kernel` with BYTES of dynamic LDS; above 64 KiB the kernel is opted in first, once per device
// (the flag belongs to this instantiation, that is to the kernel).
template <auto Kernel, int BYTES, typename... A>
int launch_lds(dim3 grid, dim3 block, hipStream_t st, const char *fn, A... args) {
    static std::atomic<unsigned long long> lds_ok{0};
    if (BYTES > 64 * 1024) {
        const int rc = rtk_ensure_dynamic_lds(reinterpret_cast<const void *>(Kernel), BYTES, lds_ok, fn);
        if (rc != RTK_OK) return rc;
    }
    RTK_LAUNCH_SCORE(Kernel, grid, block, BYTES, st, args...);
    return RTK_OK;
}

}  // namespace
