// Filtered top-k link prediction without the score matrix (rtk_score_topk_*): the k best objects of every query among
// rows [col0, col0 + n_local) of O, exactly what rtk_select_topk_f32 gives on the probabilities of the stored score
// kernels, with nothing of size batch x n_local in memory.
//
//   step 1  tmax_kernel    entity-stationary, the sweep of rtk_score_rank_kernel.h: a workgroup of 4 waves keeps 128
//                          converted rows of O as Frag B fragments and sweeps the query tiles through a
//                          double-buffered LDS stage.  Each 32 x 32 tile of probabilities is reduced to its row maximum
//                          over the tile's 128 entities -- over the 32 entity lanes by the halving butterfly, over the
//                          4 waves through LDS -- and one float per (query, entity tile) goes to tmax (B, n_tiles).
//   step 2  patch_kernel   per query with a filter list: every entity tile that holds a filtered object of the query is
//                          scored again for that query alone (a tile whose 32 A rows are all query d, as target_kernel),
//                          the query's filtered objects are masked and the corrected maximum overwrites tmax[d, tile].
//   step 3  rtk_select_topk_f32 on tmax: the k_t = min(k, n_tiles) best tiles of every query, ties by lower tile.
//   step 4  gather_kernel  step 2's scoring with another epilogue: the 128 probabilities and global ids of every
//                          selected tile (-inf, -1 for filtered rows and rows past the block) into (B, 128 k_t)
//                          candidate matrices, the tiles of a query in ascending tile order.
//   step 5  rtk_select_topk_f32 in merge mode on the candidates: (values, ids), (B, k).
//
// Why k tiles are enough.  Order tiles by (eligible maximum descending, tile ascending) and elements by (value
// descending, id ascending).  If an eligible element e lies in a tile that is not among the first k tiles, k tiles
// precede its tile; the maximum of each is a distinct eligible element that precedes e (a larger value, or an equal value
// in a lower tile and hence a lower id).  So e is not among the k best, and the first min(k, n_tiles) tiles hold the
// filtered top k.  The maxima must therefore exclude the filtered objects (step 2).  The candidates are laid out in
// ascending id order because merge mode splits a tie at the cut-off in column order.
//
// The maxima are taken on the select kernel's keys (rtk_topk_key.h), so a NaN wins its tile as it wins the select; a
// masked or absent row has the key of -inf, below every probability.  Every probability comes from Frag<T, KS>
// (rtk_score_rank_kernel.h): its bits depend on (query row, entity row, c) only, so steps 1, 2 and 4 see the same
// numbers, and any partition of [0, n_ent) into blocks sees them too.  Each tmax entry has one writer per step (step 1:
// the workgroup that owns the entity tile and the query range; step 2: wave tile % TS_UQ of the query), steps are
// stream-ordered, there are no float atomics: repeated calls give the same bits.
#include "rtk_common.h"
#include "rtk_pack.h"
#include "rtk_score_rank_kernel.h"
#include "rtk_score_select.h"
#include "rtk_topk_key.h"

namespace {

constexpr int TS_WAVES = SW_WAVES;             // waves per workgroup of the sweep: 128 entity rows per tile
constexpr int TS_TILE = SW_TILE;
constexpr int TS_UQ = 4;                       // patch waves per query (one workgroup)
constexpr int TS_KMAX = 128;
constexpr uint32_t TS_KEY_NINF = 0x007fffffu;  // sel_key(-inf): a masked or absent row

// LDS of tmax_kernel: two query tiles (nothing travels with them), then the waves' maxima
template <typename T, int KS>
struct MaxLds {
    static constexpr int TILE = (int)tile_bytes<T, KS>();
    static constexpr int RED = 2 * TILE;            // [2][TS_WAVES][32] keys
    static constexpr int RED_BUF = TS_WAVES * 32 * 4;
    static constexpr int TOTAL = RED + 2 * RED_BUF;
};

// What tmax_kernel does with the sweep: the row maximum of each 32 x 32 tile of probabilities, on the select kernel's
// keys, over the 32 entity lanes by the butterfly and over the 4 waves through LDS.
template <typename T, int KS, int SG>
struct MaxSweep {
    typedef MaxLds<T, KS> L;
    static constexpr int EXTRA = 0;
    int B, n_tiles;
    float *__restrict__ tmax;

    __device__ __forceinline__ void load_extra(SweepLane, int) const {}
    __device__ __forceinline__ void store_extra(SweepLane, int) const {}
    __device__ __forceinline__ void begin_tile() const {}
    __device__ __forceinline__ void end_tile(SweepLane, int) const {}
    __device__ __forceinline__ void score(SweepLane ln, const Frag<T, KS> &f, const f32x16 &acc,
                                          const unsigned char *buf, int cur, int, bool valid, int) const {
        const int wave = ln.wave, r = ln.r, h = ln.h;
        uint32_t key[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int rw = acc_row(4 * g, h);
            f32x4 sr4 = {1.f, 1.f, 1.f, 1.f};
            if (Frag<T, KS>::PLANES == 2) sr4 = *reinterpret_cast<const f32x4 *>(buf + rw * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 4 * g + q;
                key[e] = valid ? sel_key(f.template prob<SG>(acc[e], sr4[q])) : TS_KEY_NINF;
            }
        }
        const uint32_t m = reduce16(key, r, RedMax());
        if (!(r & 1)) reinterpret_cast<uint32_t *>(sweep_lds + L::RED + cur * L::RED_BUF)[wave * 32 + red_row(r, h)] = m;
    }
    // query tile i of the range is written by wave i % TS_WAVES, the waves' maxima taken in wave order
    __device__ __forceinline__ void publish(SweepLane ln, int cur, int i, int mt, int, int tile, bool) const {
        const int wave = ln.wave, r = ln.r, h = ln.h;
        if (wave == (i & (TS_WAVES - 1)) && h == 0) {
            const int d = mt * 32 + r;
            if (d < B) {
                const uint32_t *rc = reinterpret_cast<const uint32_t *>(sweep_lds + L::RED + cur * L::RED_BUF);
                const uint32_t s = max(max(rc[r], rc[32 + r]), max(rc[64 + r], rc[96 + r]));
                tmax[(int64_t)d * n_tiles + tile] = sel_value(s, float());
            }
        }
    }
};

// Step 1.  Workgroup (slot, qs): entity tiles slot, slot + n_slots, ...; query tiles of range qs.
template <typename T, int KS, int SG>
__global__ __launch_bounds__(64 * TS_WAVES, 2) void tmax_kernel(const unsigned char *__restrict__ qp, int B,
                                                                const T *__restrict__ O, int n_local, int c, int n_slots,
                                                                int qsplit, float *__restrict__ tmax, bool vec) {
    MaxSweep<T, KS, SG> pol{B, (n_local + TS_TILE - 1) / TS_TILE, tmax};
    sweep<T, KS, SG>(pol, qp, B, O, n_local, c, vec, n_slots, qsplit);
}

// One query against one entity tile, by one wave: QueryRow's scoring of the tile's four groups of 32 rows, and the
// query's CSR segment as a mask on them.
template <typename T, int KS, int SG>
struct QueryTile : QueryRow<T, KS> {
    const int64_t *obj;                            // the query's CSR segment [e_lo, e_hi), global ids
    int64_t e_lo, e_hi, keep;

    // the local tile of a CSR entry that takes part in the filter, else -1
    __device__ __forceinline__ int tile_of(int64_t jr, int col0, int n_local) const {
        const int64_t jl = jr - col0;
        return (jr != keep && jl >= 0 && jl < n_local) ? (int)(jl / TS_TILE) : -1;
    }
    // p[w], ok[w] of row tile * 128 + 32 w + r (meaningful in the lanes h == 0): the probability and whether the row
    // is in the block and not one of the query's filtered objects
    __device__ __forceinline__ void score_tile(const T *__restrict__ O, int n_local, int c, int col0, int tile, int lane,
                                               bool vec, float (&p)[4], bool (&ok)[4]) const {
        const int r = lane & 31, h = lane >> 5;
        uint32_t m[4] = {0u, 0u, 0u, 0u};          // the tile's filtered rows, one bit each
        for (int64_t base = e_lo; base < e_hi; base += 64) {       // wave-uniform
            const int64_t i = base + lane;
            const int64_t jr = i < e_hi ? obj[i] : -1;
            if (i < e_hi && tile_of(jr, col0, n_local) == tile) {
                const int b = (int)(jr - col0) - tile * TS_TILE;
#pragma unroll
                for (int w = 0; w < 4; ++w)
                    if ((b >> 5) == w) m[w] |= 1u << (b & 31);
            }
        }
        if (e_hi > e_lo) {
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m[w] |= (uint32_t)__shfl_xor((int)m[w], o);
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int jl = tile * TS_TILE + 32 * w + r;
            p[w] = 0.f;
            ok[w] = false;
            if (tile * TS_TILE + 32 * w >= n_local) continue;      // wave-uniform: the block ends before these rows
            Frag<T, KS> f;
            p[w] = this->template score<SG>(f, O, min(jl, n_local - 1), c, h, vec);
            ok[w] = jl < n_local && !((m[w] >> r) & 1u);
        }
    }
};

// Step 2: one workgroup of TS_UQ waves per query; wave u corrects the tiles T with T % TS_UQ == u that hold a filtered
// object of the query, each once (at the first CSR entry that names the tile).
template <typename T, int KS, int SG>
__global__ __launch_bounds__(64 * TS_UQ) void patch_kernel(const unsigned char *__restrict__ qp, int B,
                                                           const T *__restrict__ O, int n_local, int c, int col0,
                                                           const int64_t *__restrict__ pair_slot,
                                                           const int64_t *__restrict__ pair_ptr,
                                                           const int64_t *__restrict__ pair_obj,
                                                           const int64_t *__restrict__ keep_idx, float *__restrict__ tmax,
                                                           bool vec) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int d = (int)blockIdx.x, u = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_tiles = (n_local + TS_TILE - 1) / TS_TILE;
    const int64_t s = pair_slot[d];
    if (s < 0) return;
    QueryTile<T, KS, SG> q;
    q.obj = pair_obj;
    q.e_lo = pair_ptr[s];
    q.e_hi = pair_ptr[s + 1];
    q.keep = keep_idx ? keep_idx[d] : -1;
    if (q.e_hi <= q.e_lo) return;
    bool loaded = false;
    for (int64_t base = q.e_lo; base < q.e_hi; base += 64) {       // wave-uniform
        const int64_t i = base + lane;
        int tl = i < q.e_hi ? q.tile_of(pair_obj[i], col0, n_local) : -1;
        if (tl >= 0 && tl % TS_UQ != u) tl = -1;
        unsigned long long todo = __ballot(tl >= 0);
        while (todo) {
            const int first = __builtin_ctzll(todo);
            const int tile = __shfl(tl, first);
            // an earlier 64-entry chunk that names the tile has corrected it already
            bool seen = false;
            for (int64_t b2 = q.e_lo; b2 < base && !seen; b2 += 64)
                seen = __ballot(q.tile_of(pair_obj[b2 + lane], col0, n_local) == tile) != 0;
            if (!seen) {
                if (!loaded) {
                    q.load(qp, d, h);
                    loaded = true;
                }
                float p[4];
                bool ok[4];
                q.score_tile(O, n_local, c, col0, tile, lane, vec, p, ok);
                uint32_t m = TS_KEY_NINF;
#pragma unroll
                for (int w = 0; w < 4; ++w) m = max(m, ok[w] ? sel_key(p[w]) : TS_KEY_NINF);
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
                if (lane == 0) tmax[(int64_t)d * n_tiles + tile] = sel_value(m, float());
            }
            if (tl == tile) tl = -1;
            todo = __ballot(tl >= 0);
        }
    }
}

// Step 4: wave (d, s) scores tile tile_ids[d, s] for query d and writes its 128 candidates at the tile's position in
// ascending tile order among the query's selected tiles.
template <typename T, int KS, int SG>
__global__ __launch_bounds__(64 * TS_WAVES) void gather_kernel(const unsigned char *__restrict__ qp, int B,
                                                               const T *__restrict__ O, int n_local, int c, int col0,
                                                               const int64_t *__restrict__ pair_slot,
                                                               const int64_t *__restrict__ pair_ptr,
                                                               const int64_t *__restrict__ pair_obj,
                                                               const int64_t *__restrict__ keep_idx,
                                                               const int64_t *__restrict__ tile_ids, int k_t,
                                                               float *__restrict__ cand_val, int64_t *__restrict__ cand_id,
                                                               bool vec) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t w_id = (int64_t)blockIdx.x * TS_WAVES + (int64_t)(threadIdx.x >> 6);
    const int d = __builtin_amdgcn_readfirstlane((int)(w_id / k_t)), sl = __builtin_amdgcn_readfirstlane((int)(w_id % k_t));
    if (d >= B) return;
    const int n_tiles = (n_local + TS_TILE - 1) / TS_TILE;
    const int64_t *ids = tile_ids + (int64_t)d * k_t;
    const int64_t mine = ids[sl];
    const bool real = mine >= 0 && mine < n_tiles;
    // position: the real tiles in ascending order, then the others (none with the host's k_t <= n_tiles) in list order
    int pos = 0;
    for (int j0 = 0; j0 < k_t; j0 += 64) {                         // wave-uniform
        const int j = j0 + lane;
        bool before = false;
        if (j < k_t) {
            const int64_t o = ids[j];
            const bool o_real = o >= 0 && o < n_tiles;
            before = real ? (o_real && o < mine) : (o_real || j < sl);
        }
        pos += __popcll(__ballot(before));
    }
    const int64_t at = ((int64_t)d * k_t + pos) * TS_TILE;
    if (!real) {
        for (int i = lane; i < TS_TILE; i += 64) {
            cand_val[at + i] = -INFINITY;
            cand_id[at + i] = -1;
        }
        return;
    }
    QueryTile<T, KS, SG> q;
    const int64_t s = pair_slot ? pair_slot[d] : -1;
    q.obj = pair_obj;
    q.e_lo = s >= 0 ? pair_ptr[s] : 0;
    q.e_hi = s >= 0 ? pair_ptr[s + 1] : 0;
    q.keep = keep_idx ? keep_idx[d] : -1;
    q.load(qp, d, h);
    float p[4];
    bool ok[4];
    const int tile = (int)mine;
    q.score_tile(O, n_local, c, col0, tile, lane, vec, p, ok);
    if (h == 0) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            cand_val[at + 32 * w + r] = ok[w] ? p[w] : -INFINITY;
            cand_id[at + 32 * w + r] = ok[w] ? (int64_t)col0 + tile * TS_TILE + 32 * w + r : -1;
        }
    }
}

// [0, 256): the error word's header; the tile maxima; the selected tiles' values and ids; the candidates
struct TopkWs {
    int64_t n_tiles, k_t;
    size_t tmax, tval, tid, cval, cid, total;
};
TopkWs layout_of(int64_t batch, int64_t n_local, int k) {
    TopkWs L;
    L.n_tiles = rtk_cdiv(n_local, TS_TILE);
    L.k_t = k < L.n_tiles ? k : L.n_tiles;
    const size_t b = (size_t)(batch > 0 ? batch : 0), kt = (size_t)L.k_t;
    L.tmax = 256;
    L.tval = L.tmax + rtk_align_up(b * (size_t)L.n_tiles * 4, 256);
    L.tid = L.tval + rtk_align_up(b * kt * 4, 256);
    L.cval = L.tid + rtk_align_up(b * kt * 8, 256);
    L.cid = L.cval + rtk_align_up(b * kt * TS_TILE * 4, 256);
    L.total = L.cid + rtk_align_up(b * kt * TS_TILE * 8, 256);
    return L;
}

bool shape_ok(int dtype, int c, int k) {
    if (k < 1 || k > TS_KMAX || c < 1) return false;
    if (dtype == RTK_F32) return c <= 16 * SW_MAX_KS_F32 && c % 4 == 0;
    return dtype == RTK_BF16 && c <= 16 * SW_MAX_KS_BF16;
}

template <typename T, int KS, int SG>
int launch_topk(const unsigned char *qp, int B, const T *O, int n_local, int c, int col0, const int64_t *pair_slot,
                const int64_t *pair_ptr, const int64_t *pair_obj, const int64_t *keep_idx, int k, float *values_out,
                int64_t *ids_out, unsigned char *ws, hipStream_t st, const char *fn) {
    const TopkWs L = layout_of(B, n_local, k);
    const SweepGrid g = grid_of(B, n_local, SW_SLOTS);
    const int n_tiles = (int)L.n_tiles, k_t = (int)L.k_t;
    float *tmax = reinterpret_cast<float *>(ws + L.tmax);
    float *tval = reinterpret_cast<float *>(ws + L.tval);
    int64_t *tid = reinterpret_cast<int64_t *>(ws + L.tid);
    float *cval = reinterpret_cast<float *>(ws + L.cval);
    int64_t *cid = reinterpret_cast<int64_t *>(ws + L.cid);
    const bool vec = vec_rows(O, c);

    int rc = launch_lds<&tmax_kernel<T, KS, SG>, MaxLds<T, KS>::TOTAL>(dim3((unsigned)(g.n_slots * g.qsplit)),
                                                                       dim3(64 * TS_WAVES), st, fn, qp, B, O, n_local, c,
                                                                       g.n_slots, g.qsplit, tmax, vec);
    if (rc != RTK_OK) return rc;
    if (pair_slot)
        hipLaunchKernelGGL((patch_kernel<T, KS, SG>), dim3((unsigned)B), dim3(64 * TS_UQ), 0, st, qp, B, O, n_local, c, col0,
                           pair_slot, pair_ptr, pair_obj, keep_idx, tmax, vec);
    rc = rtk_check_launch(fn);
    if (rc != RTK_OK) return rc;
    rc = rtk_select_topk_f32(tmax, B, n_tiles, n_tiles, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, k_t, tval, tid,
                             nullptr, 0, st);
    if (rc != RTK_OK) return rc;
    hipLaunchKernelGGL((gather_kernel<T, KS, SG>), dim3((unsigned)rtk_cdiv((int64_t)B * k_t, TS_WAVES)), dim3(64 * TS_WAVES), 0,
                       st, qp, B, O, n_local, c, col0, pair_slot, pair_ptr, pair_obj, keep_idx, tid, k_t, cval, cid, vec);
    rc = rtk_check_launch(fn);
    if (rc != RTK_OK) return rc;
    const int64_t n_cand = (int64_t)k_t * TS_TILE;
    return rtk_select_topk_f32(cval, B, n_cand, n_cand, 0, cid, n_cand, nullptr, nullptr, nullptr, nullptr, k, values_out,
                               ids_out, nullptr, 0, st);
}

template <typename T>
int score_topk(const char *fn, const void *q_packed, int64_t batch, int c, const T *O, int64_t n_local, int64_t col0,
               int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
               const int64_t *keep_idx, int k, unsigned flags, float *values_out, int64_t *ids_out, void *workspace,
               size_t ws_bytes, void *stream) {
    const auto own = [&]() -> int {
        RTK_REQUIRE(!pair_slot || (pair_ptr && pair_obj), RTK_ERR_BAD_ARG, "%s: pair_slot without the CSR arrays", fn);
        RTK_REQUIRE(k >= 1 && k <= TS_KMAX, RTK_ERR_BAD_ARG, "%s: k = %d outside [1, %d]", fn, k, TS_KMAX);
        RTK_REQUIRE(batch * (int64_t)TS_KMAX < (1ll << 31), RTK_ERR_UNSUPPORTED,
                    "%s: batch = %lld too large for one call (split the queries)", fn, (long long)batch);
        return RTK_OK;
    };
    const int rc = check_block(fn, q_packed && values_out && ids_out, batch, c, O, n_local, col0, n_ent, own,
                               (1ll << 31) - 256, flags, "the top k is", workspace, ws_bytes,
                               [&] { return layout_of(batch, n_local, k).total; });
    if (rc != RTK_OK || batch == 0) return rc;
    return dispatch<T>(fn, c, flags, [&](auto K, auto SG) {
        return launch_topk<T, K.value, SG.value>((const unsigned char *)q_packed, (int)batch, O, (int)n_local, c, (int)col0,
                                                 pair_slot, pair_ptr, pair_obj, keep_idx, k, values_out, ids_out,
                                                 (unsigned char *)workspace, (hipStream_t)stream, fn);
    });
}

}  // namespace

extern "C" size_t rtk_score_topk_workspace_bytes(int dtype, int64_t batch, int64_t n_local, int c, int k) {
    if (batch < 0 || n_local < 1 || !shape_ok(dtype, c, k)) return 0;
    return layout_of(batch, n_local, k).total;
}

extern "C" int rtk_score_topk_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                  int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                  const int64_t *pair_obj, const int64_t *keep_idx, int k, unsigned flags,
                                  float *values_out, int64_t *ids_out, void *workspace, size_t ws_bytes, void *stream) {
    return score_topk<float>("rtk_score_topk_f32", q_packed, batch, c, O_local, n_local, col0, n_ent, pair_slot, pair_ptr,
                             pair_obj, keep_idx, k, flags, values_out, ids_out, workspace, ws_bytes, stream);
}

extern "C" int rtk_score_topk_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                   int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                   const int64_t *pair_obj, const int64_t *keep_idx, int k, unsigned flags,
                                   float *values_out, int64_t *ids_out, void *workspace, size_t ws_bytes, void *stream) {
    return score_topk<rtk_bf16>("rtk_score_topk_bf16", q_packed, batch, c, (const rtk_bf16 *)O_local, n_local, col0, n_ent,
                                pair_slot, pair_ptr, pair_obj, keep_idx, k, flags, values_out, ids_out, workspace, ws_bytes,
                                stream);
}
