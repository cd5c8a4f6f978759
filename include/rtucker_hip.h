/*
 * rtucker_hip.h -- C ABI of librtucker_hip.so: R-TuckER's 1-vs-all Tucker scoring
 * path for AMD MI355X (gfx950 / CDNA4), hand-written HIP kernels.
 *
 * The reference (johanDDC/R-TuckER) has no native boundary: the path is the
 * Python closure  score_fn = model(subject_idx, relation_idx);  P = score_fn(T)
 * (src/model/asymmetric/R_TuckER.py:41-50, src/model/symmetric/R_TuckER.py:38-47).
 * This header is the boundary a maintainer binds instead of the five torch ops
 * inside that closure (INTEGRATION.md shows the ctypes stub).  Each entry point
 * below cites the reference lines it replaces.
 *
 * Conventions
 *  - plain C symbols, no C++/torch types; every pointer is a DEVICE pointer
 *    (hipMalloc'd / torch tensor .data_ptr()) unless the name says "host";
 *  - row-major, contiguous operands; sizes are element counts;
 *  - core axis order is (relation a, subject b, object c)  [train.py:41,
 *    asymmetric/R_TuckER.py:20-23];  factors R:(nR,a)  S:(nS,b)  O:(N,c);
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream); every call
 *    only ENQUEUES work on it: no allocation, no synchronisation, no hidden
 *    state besides a thread-local last-error string -> graph-capturable;
 *  - scratch memory is caller-owned: query its size with rtk_workspace_bytes(),
 *    pass it in; the same workspace must not be used by two in-flight calls;
 *  - return value: 0 = RTK_OK, negative = rtk_status (nothing was enqueued).
 *    Index values are range-checked ON DEVICE: an out-of-range id never reads
 *    out of bounds (it is clamped) and raises bit 0 of the 32-bit word at the
 *    start of the workspace, which rtk_read_error_flag() fetches (synchronising).
 *    (Reference behaviour: torch raises IndexError / device assert.)
 */
#ifndef RTUCKER_HIP_H
#define RTUCKER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rtk_status {
    RTK_OK = 0,
    RTK_ERR_BAD_ARG = -1,      /* null pointer, non-positive size, b != c ...        */
    RTK_ERR_WORKSPACE = -2,    /* workspace missing or smaller than required        */
    RTK_ERR_UNSUPPORTED = -3,  /* shape outside what the kernels implement          */
    RTK_ERR_LAUNCH = -4        /* hipGetLastError() after a launch was not success  */
} rtk_status;

typedef enum rtk_dtype {
    RTK_F32 = 0,   /* fp32 operands, fp32 scores (reference dtype, R_TuckER.py:23)   */
    RTK_BF16 = 1   /* bf16 operands, fp32 accumulate, fp32 scores                    */
} rtk_dtype;

/* flags for the score stage */
#define RTK_SCORE_SIGMOID 1u      /* apply sigmoid (R_TuckER.py:48); else raw logits  */
#define RTK_SCORE_EXACT_F32 2u    /* fp32 operands: force the exact-fp32 MFMA kernel   */
                                  /* instead of the split-fp16 (hi/lo) MFMA kernel     */
/*
 * Precision of the default fp32 score kernel (rtk_score_packed_f32, "split-fp16"): every operand row
 * (a query vector v_d, an entity row O[j]) is scaled by a power of two so that its LARGEST element
 * lands in [2^14, 2^15) and each element is split x = hi + lo into two fp16 values (~22 significand
 * bits relative to the ROW MAXIMUM); v.o ~= vh.oh + vh.ol + vl.oh, accumulated in fp32 (the vl.ol
 * term, 2^-22 relative, is dropped).  The guarantee is therefore NORMWISE PER ROW, not element-wise:
 *     |dz[d,j]|  <~  2^-21 * K * max|v_d| * max|O_j|
 * (typical; the worst case of the split alone is (2^-19 + 2^-22) * K * max|v_d| * max|O_j|: per k, lo is rounded to
 * within 2^-11 ulp_fp16(hi) <= 2^-7 of the scaled element, against a factor below 2^15, on either side, plus the
 * dropped |vl| |ol| <= 2^6, over max * max >= 2^28; tests/test_split_cases_host.py)
 * -- elements much smaller than their row's maximum lose RELATIVE precision: an element keeps all 22
 * bits while its scaled value is at least 2^-2 (2^-16 of a row maximum of exactly 2^14, 2^-17 of one just below
 * 2^15), then one bit less per factor of two (lo becomes an fp16 subnormal, then zero) to 11
 * bits at 2^-28, and is dropped entirely below 2^-39 of the row maximum (hi a subnormal, then zero) -- which
 * does not matter for a dot product dominated by the large elements but is not what an exact fp32
 * product gives for rows of extreme dynamic range.  The matrix core takes fp16 subnormal operands at their value (no
 * flush): on operands whose partial sums cannot round, all three kernels return (vh.oh + vh.ol + vl.oh) 2^-(sh_v + sh_o)
 * of the numpy model in tests/golden/split_cases.py bit for bit, subnormal lo planes included
 * (tests/test_gpu_split_exact.py).
 * Range: the shift is 14 - floor(log2 max), clamped to +-100 (rtk_pack_shift), so a row keeps this precision for
 * 2^-86 <= max < 2^115.  Below 2^-86 the row is scaled by 2^100 only and its elements lose bits as small elements
 * do (all of them below 2^-125); from about 2^116 on (max * 2^-100 > 65504) hi overflows fp16 and the scores of that
 * row or column are not finite.  An all-zero row, or one whose maximum is not finite, gets the shift 0.  The two row
 * factors are powers of two and the unscale multiplies them exactly as long as z itself is a normal fp32 number and
 * sh_v + sh_o <= 149: the ws kernel forms 2^-sh_v * 2^-sh_o first, which is zero beyond that (max|v_d| * max|O_j|
 * below about 2^-121), where v3 and cg, which multiply one factor after the other, still return a value.  Checked
 * bit for bit with row maxima from 2^-60 to 2^60 on both sides, wherever z's unit is a normal number.
 * Measured: the same error against float64 as the
 * reference's CPU sgemm at rank (10,200,200) (3-5e-6 relative; tests/test_gpu_parity.py,
 * test_wide_dynamic_range_rows).  RTK_SCORE_EXACT_F32 selects v_mfma_f32_32x32x2_f32 (bitwise an
 * fmaf chain) at 1/5 of the throughput when element-wise fp32 behaviour is required.
 */
#define RTK_SCORE_SIGMOID_FAST 4u /* with RTK_SCORE_SIGMOID: 1 / (1 + 2^(-z log2 e)) on  */
                                  /* v_exp_f32 + v_rcp_f32 (1 ulp each) instead of expf */
                                  /* + IEEE divide                                      */
#define RTK_SCORE_OUT_BF16 8u     /* bf16 operand entry points, with SIGMOID | SIGMOID_FAST:   */
                                  /* `out` holds bf16 scores (what the reference's bf16 model */
                                  /* returns), ld_out counts bf16 elements; pass the pointer  */
                                  /* through the float* parameter                              */

/* Which fp32 split-fp16 score kernel runs (rtk_score_packed_f32, rtk_score_1vN_f32); 0 = by shape.  The kernels
 * give the same scores up to the summation order inside a dot product; the hints exist for A/B runs and so that
 * the tests can put every kernel on every shape.  A hinted kernel that does not cover the shape falls through to
 * the next one (cg: c <= 208, c % 4 == 0; ws: the same; v3: c <= 512). */
#define RTK_SCORE_KERNEL_MASK 0x300u
#define RTK_SCORE_KERNEL_CG 0x100u  /* column-group kernel (csrc/rtk_score_cg_kernel.h), on any entity count    */
#define RTK_SCORE_KERNEL_WS 0x200u  /* wave-specialised persistent kernel (csrc/rtk_score_ws_kernel.h)           */
#define RTK_SCORE_KERNEL_V3 0x300u  /* two workgroups per CU, every wave does everything (rtk_score_split_kernel.h) */

/* Host-only queries of the rule rtk_score_packed_f32 follows (no device is touched; valid without a GPU), for a
 * 16-byte-aligned O, n_local entities, object rank c <= 512 and the kernel hint bits of `flags`:
 * rtk_score_kernel_f32 returns the RTK_SCORE_KERNEL_* value of the kernel that runs;
 * rtk_score_fifth_group_columns_f32 returns how many of the n_local entity columns the column-group kernel computes
 * as a K-split fifth group of its set (four K-range chains added in a fixed order instead of one chain: these scores
 * may differ in the last bits from an entity-sharded run), and if `mask` is not NULL sets mask[j] to 1 for those
 * columns and 0 for the others (n_local bytes).  0 unless the column-group kernel runs.  Both return
 * RTK_ERR_BAD_ARG for shapes rtk_score_packed_f32 does not take. */
int rtk_score_kernel_f32(int64_t n_local, int c, unsigned flags);
int64_t rtk_score_fifth_group_columns_f32(int64_t n_local, int c, unsigned flags, unsigned char *mask);

int rtk_version(void);
const char *rtk_last_error_string(void);

/* Bytes of workspace the calls below need for these sizes (upper bound, 256-B aligned). */
size_t rtk_workspace_bytes(int dtype, int64_t batch, int64_t n_rel, int a, int b, int c);

/* Fetches and clears the device error word of a workspace (hipStreamSynchronize
 * on `stream` first).  Bit 0: relation/subject index out of range.  Bit 1: a
 * candidate id of rtk_score_candidates_* out of range. */
int rtk_read_error_flag(void *workspace, void *stream, uint32_t *host_flag_out);

/*
 * Stage 1: query vectors  v[d,:] = S[h_d,:] . ( G x_0 R[r_d,:] )        (B x c)
 * replaces asymmetric/R_TuckER.py:43-46 (two gathers, einsum "abc,da->dbc", bmm)
 * and symmetric/R_TuckER.py:40-43 (pass E as S).  Requires b == c like the
 * reference's .view(-1, b) -> RTK_ERR_BAD_ARG otherwise.
 *   v_out    : fp32 (B x c), may be NULL
 *   q_packed : "query planes" consumed by rtk_score_packed_*, may be NULL;
 *              size rtk_packed_query_bytes(dtype, B, c)
 * Internally: relation tables M_u = G x_0 R[u] for the distinct relations of the
 * batch, then v_d = S[h_d] . M_{r_d}  (the reference's summation order).
 */
int rtk_query_vectors_f32(const float *core, int a, int b, int c,
                          const float *R, int64_t n_rel,
                          const float *S, int64_t n_sub,
                          const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                          float *v_out, void *q_packed,
                          void *workspace, size_t workspace_bytes, void *stream);

size_t rtk_packed_query_bytes(int dtype, int64_t batch, int c);

/*
 * Packed query planes from fp32 query vectors computed elsewhere (entity-sharded scoring with stage 1
 * split over the ranks: each rank contracts a slice of the batch, the (batch x c) vectors are
 * all-gathered, every rank packs them and scores its entity shard with rtk_score_packed_*).  Same
 * arithmetic as the packing inside rtk_query_vectors_* (bit-identical planes).  dtype: rtk_dtype of
 * the score kernel that will consume them.
 */
int rtk_pack_query_vectors(const float *v, int64_t batch, int c, int dtype, void *q_packed, void *stream);

/*
 * Stage 1 split at the relation tables, for callers whose parameters stay fixed over many batches
 * (the evaluation loop, train.py:107-121: extract_tensor(model) is the same tensor for every batch).
 * The einsum of asymmetric/R_TuckER.py:45 applied to ALL relation rows,
 *     tables[u, :, :] = sum_a R[u, a] * G[a, :, :]          (n_rel x b x c, fp32)
 * depends on the parameters only:
 *   rtk_relation_tables_{f32,bf16}            build it once per parameter version
 *                                             (bytes: rtk_relation_tables_bytes; scratch:
 *                                             rtk_relation_tables_workspace_bytes, >= 256)
 *   rtk_query_vectors_from_tables_{f32,bf16}  per batch: v_d = S[h_d] . tables[r_d]   (R_TuckER.py:43-46
 *                                             given the tables); same outputs as rtk_query_vectors_*;
 *                                             workspace rtk_from_tables_workspace_bytes, whose first
 *                                             word is the sticky error word like the main workspace's.
 * Same summation order as rtk_query_vectors_*: the results are bit-identical to the uncached path.
 * `tables` must be 256-byte aligned.
 */
size_t rtk_relation_tables_bytes(int64_t n_rel, int b, int c);
size_t rtk_relation_tables_workspace_bytes(int dtype, int64_t n_rel, int a, int b, int c);
size_t rtk_from_tables_workspace_bytes(int64_t batch, int64_t n_rel);

int rtk_relation_tables_f32(const float *core, int a, int b, int c, const float *R, int64_t n_rel,
                            float *tables, void *workspace, size_t workspace_bytes, void *stream);
int rtk_relation_tables_bf16(const void *core, int a, int b, int c, const void *R, int64_t n_rel,
                             float *tables, void *workspace, size_t workspace_bytes, void *stream);

int rtk_query_vectors_from_tables_f32(const float *tables, int64_t n_rel, int b, int c,
                                      const float *S, int64_t n_sub,
                                      const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                                      float *v_out, void *q_packed,
                                      void *workspace, size_t workspace_bytes, void *stream);
int rtk_query_vectors_from_tables_bf16(const float *tables, int64_t n_rel, int b, int c,
                                       const void *S, int64_t n_sub,
                                       const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                                       float *v_out, void *q_packed,
                                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same step restricted to the queries whose relation id is congruent to `part` modulo `n_parts`: their rows of
 * v_out (B x c fp32, required) are written, every other row is left untouched.  This is stage 1 split over the ranks
 * of an entity-sharded run BY RELATION: a rank then streams only the tables of its own relations
 * (1/n_parts of rtk_relation_tables_bytes instead of nearly all of it when the batch is split by position: at
 * BASELINE.json configs[4], 8192 queries over 1000 relations, a batch slice of 1024 queries still touches ~640
 * tables of 1 MB); the B x c vectors are completed by one all-reduce(SUM) over buffers zeroed before the call --
 * every row is non-zero on exactly one rank, so the sum is exact -- and packed with rtk_pack_query_vectors.
 */
int rtk_query_vectors_from_tables_part_f32(const float *tables, int64_t n_rel, int b, int c,
                                           const float *S, int64_t n_sub,
                                           const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                                           int part, int n_parts, float *v_out,
                                           void *workspace, size_t workspace_bytes, void *stream);
int rtk_query_vectors_from_tables_part_bf16(const float *tables, int64_t n_rel, int b, int c,
                                            const void *S, int64_t n_sub,
                                            const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                                            int part, int n_parts, float *v_out,
                                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Stage 2: scores  out[d, j] = sigmoid( v[d,:] . O[j,:] )   for j < n_local
 * replaces asymmetric/R_TuckER.py:47-48 ( @ T.factors[2].T ; sigmoid ) and
 * symmetric/R_TuckER.py:44-45.  `O` is the (shard of the) entity matrix,
 * (n_local x c) row-major; `out` has leading dimension ld_out >= n_local.
 * rtk_score_f32        : exact fp32 MFMA (v_mfma_f32_32x32x2_f32), v in fp32.
 * rtk_score_packed_f32 : split-fp16 MFMA path, v given as packed query planes.
 */
int rtk_score_f32(const float *v, int64_t batch, int c,
                  const float *O, int64_t n_local,
                  float *out, int64_t ld_out, unsigned flags, void *stream);

int rtk_score_packed_f32(const void *q_packed, int64_t batch, int c,
                         const float *O, int64_t n_local,
                         float *out, int64_t ld_out, unsigned flags, void *stream);

/*
 * Both stages: the whole closure body, asymmetric/R_TuckER.py:43-48.
 * out (B x ld_out) receives sigmoid scores (or logits without RTK_SCORE_SIGMOID)
 * against the n_local rows of O.  For the symmetric model pass S == O == E.
 */
int rtk_score_1vN_f32(const float *core, int a, int b, int c,
                      const float *R, int64_t n_rel,
                      const float *S, int64_t n_sub,
                      const float *O, int64_t n_local,
                      const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                      float *out, int64_t ld_out, unsigned flags,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * bf16 operand path (BASELINE.json configs[2], [4]): core, R, S, O are bf16 (raw 16-bit
 * storage, torch.bfloat16), all accumulation is fp32, the query vectors are rounded to bf16
 * before the score product (v_mfma_f32_32x32x16_bf16), scores are fp32.  Same argument
 * meaning, workspace rules (query sizes with dtype = RTK_BF16) and reference lines as the
 * _f32 entry points above.  rtk_score_packed_bf16 forms exact products and sums the c/16
 * k-steps recursively in fp32: |z - v^.o| <= 2^-24 * 16 * ceil(c/16) * sum_k |v^_k||o_k| for the
 * bf16-rounded v^.  The k-step order depends on c alone, not on n_local, batch, the
 * logistic or the output type: a score has the same bits in every launch geometry (entity
 * shards, query subsets, cached relation tables), and bf16 scores are the fp32 ones rounded.
 */
int rtk_query_vectors_bf16(const void *core, int a, int b, int c,
                           const void *R, int64_t n_rel,
                           const void *S, int64_t n_sub,
                           const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                           float *v_out, void *q_packed,
                           void *workspace, size_t workspace_bytes, void *stream);

int rtk_score_packed_bf16(const void *q_packed, int64_t batch, int c,
                          const void *O, int64_t n_local,
                          float *out, int64_t ld_out, unsigned flags, void *stream);

int rtk_score_1vN_bf16(const void *core, int a, int b, int c,
                       const void *R, int64_t n_rel,
                       const void *S, int64_t n_sub,
                       const void *O, int64_t n_local,
                       const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                       float *out, int64_t ld_out, unsigned flags,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * General fp32 MFMA GEMM used by the backward pass and as the exact fallback:
 *   C[m,n] (+)= sum_k A(m,k) * B(n,k)
 * A(m,k) = A[m*lda + k] if a_kmajor else A[k*lda + m]; likewise B(n,k).
 * flags: RTK_SCORE_SIGMOID applies sigmoid to C.
 */
int rtk_gemm_f32(const float *A, int a_kmajor, int64_t lda,
                 const float *B, int b_kmajor, int64_t ldb,
                 float *C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                 unsigned flags, void *stream);

/* Split-K variant for short-and-wide products (K >> M, N), e.g. the backward product
 * dv = dZ . O (K = number of entities; autograd of asymmetric/R_TuckER.py:47): the K chunks are
 * computed by separate workgroups into slabs of the caller's workspace
 * (rtk_gemm_f32_splitk_workspace_bytes) and added in chunk order by a second kernel -- a fixed
 * summation order, bit-identical from run to run (no float atomics).  C contiguous (ldc == N). */
size_t rtk_gemm_f32_splitk_workspace_bytes(int64_t M, int64_t N, int splits);
int rtk_gemm_f32_splitk(const float *A, int a_kmajor, int64_t lda,
                        const float *B, int b_kmajor, int64_t ldb,
                        float *C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                        int splits, void *workspace, size_t workspace_bytes, void *stream);

/* The same product on the split-fp16 path of the forward (three f16 MFMAs per k-step on hi/lo halves,
 * fp32 accumulation) for the two B x N sized backward products of asymmetric/R_TuckER.py:47,
 * dO = dZ^T v and dv = dZ O.  amax_a / amax_b: DEVICE pointers to one float each, an UPPER BOUND of
 * max|A| and max|B| (for the BCE gradient |dZ| <= |g| / (B N) needs no pass over dZ); each operand is
 * scaled by the power of two that puts its bound just below 2^15, so an element larger than the bound
 * overflows to inf (loud), and an element keeps max(2^-22 |x|, 2^-40 bound) of absolute accuracy: the
 * result is accurate normwise, relative to max|A| max|B| K -- right for a gradient, not for an
 * orthogonalisation (use rtk_gemm_f32 there).  The power of two is 2^e, e = 14 - floor(log2 bound), taken from the
 * bound's exponent field: every normal bound up to FLT_MAX is served (e >= -113), e is capped at 100, so an operand
 * under a bound below 2^-86 is scaled by 2^100 all the same and loses bits to fp16's subnormals; a bound that is 0,
 * subnormal, inf or nan gets the scale 1 -- a subnormal operand then contributes zeros, and an operand under an inf
 * or nan bound is taken as it stands and has to lie within fp16's range itself.  The accumulator is multiplied by
 * 2^-(ea + eb) in one step where that is a normal float, else in two steps of the same sign: the result is the
 * rounded one whenever it is a normal float, whatever the two bounds are.  splits == 1: C may have any ldc >= N, no workspace;
 * splits > 1: as rtk_gemm_f32_splitk (slabs added in chunk order: deterministic). */
int rtk_gemm_sf16_splitk(const float *A, int a_kmajor, int64_t lda, const float *amax_a,
                         const float *B, int b_kmajor, int64_t ldb, const float *amax_b,
                         float *C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                         int splits, void *workspace, size_t workspace_bytes, void *stream);

/* max |x| over a rows x cols fp32 matrix with row pitch ld -> *out (one float on the device): the operand
 * bounds of rtk_gemm_sf16_splitk when the caller has no analytic one.  Order-independent (integer atomicMax
 * on the bit patterns), NaNs skipped. */
int rtk_absmax_f32(const float *x, int64_t rows, int64_t cols, int64_t ld, float *out, void *stream);

/*
 * Backward of stage 1 (autograd of asymmetric/R_TuckER.py:43-46, which the Riemannian gradient
 * differentiates through loss_fn, train.py:79-82): given dv = d loss / d v (batch x c, fp32),
 *   g_core (a,b,c) = sum_d R[r_d] (x) S[h_d] (x) dv[d]
 *   g_R (n_rel,a)  : row u = sum over the queries with r_d = u of  (G x_1 S[h_d] x_2 dv[d])
 *   g_S (n_sub,b)  : row j = sum over the queries with h_d = j of  (G x_0 R[r_d] x_2 dv[d])
 * Each output may be NULL (skipped); the others are written in full (untouched rows = 0).
 * Deterministic: fixed summation order everywhere (the row scatter adds the queries of an id in
 * increasing query order; no float atomics).  Ranks up to 1024.  Workspace:
 * rtk_query_bwd_workspace_bytes (2 * batch * a * b floats + the per-query rows).
 */
size_t rtk_query_bwd_workspace_bytes(int64_t batch, int a, int b, int c);
int rtk_query_vectors_bwd_f32(const float *core, int a, int b, int c,
                              const float *R, int64_t n_rel,
                              const float *S, int64_t n_sub,
                              const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                              const float *dv, float *g_core, float *g_R, float *g_S,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same backward without anything of size batch x a*b: neither W[d,i,j] = sum_k G[i,j,k] dv[d,k] nor the Khatri-Rao
 * operand R[r_d,i] S[h_d,j] is written.  Arguments, the NULL-output rule, refusals and return codes are those of
 * rtk_query_vectors_bwd_f32; ranks a, b, c up to 1024.  dv and the three outputs are fp32 in both entries.  The _bf16
 * entry reads core, R and S as bf16 and converts on load (exact; no fp32 copy of an operand is made): its result is the
 * _f32 entry's on the upcast operands, bit for bit.
 * Workspace (rtk_query_bwd_stream_workspace_bytes; valid without a device, 0 at batch <= 0), 256-byte aligned pieces:
 * the gathered fp32 rows R[r_d] (batch x a) and S[h_d] (batch x b), the per-query rows rows_R (batch x a) and rows_S
 * (batch x b), and the partial sums of rows_R per 128-column tile of b (ceil(b / 128) x batch x a):
 * 4 batch (2 a + 2 b + ceil(b / 128) a) bytes plus alignment.
 * THE ORDER OF THE SUMS (deterministic: no float atomics, no split that depends on the batch):
 *   W[d,i,j]     one fmaf chain over k ascending from zero (fp32 MFMA; k-tiles of 16, the last one zero-padded).  It
 *                lives in registers only.
 *   rows_S[d,j]  = sum_i W[d,i,j] R[r_d,i]: one chain fmaf(W, R[r_d,i], acc) over i ascending from zero -- the chain of
 *                rtk_query_vectors_bwd_f32, so g_S has that entry's values on every input (a zero may differ in sign).
 *   rows_R[d,i]  = sum_j W[d,i,j] S[h_d,j]: per tile of 128 columns j0 .. j0 + 127 (columns past b count as zeros),
 *                lane r = 0 .. 31 forms p_r = W[j0+r] S[j0+r], then fmaf(W[j0+r+32], S[j0+r+32], p_r), then the terms of
 *                + 64 and + 96; the 32 lane sums are combined by a butterfly, p_r += p_(r xor 16), then xor 8, 4, 2, 1;
 *                the tiles' sums are added in ascending tile order starting from tile 0's.  The bits depend on S[h_d],
 *                dv[d], the core and the tile width alone, not on the batch size nor on the query's place in the batch.
 *   g_core       rtk_core_outer_f32 on the gathered rows and dv: one chain over d ascending from zero, no split-K (so
 *                its bits differ from rtk_query_vectors_bwd_f32's where that entry splits K).
 *   g_R, g_S     the ordered row scatter of rtk_query_vectors_bwd_f32 on rows_R, rows_S (the same kernel).
 * Out-of-range ids are clamped, as in rtk_query_vectors_bwd_f32 (the forward has flagged them).
 */
size_t rtk_query_bwd_stream_workspace_bytes(int64_t batch, int a, int b, int c);
int rtk_query_vectors_bwd_stream_f32(const float *core, int a, int b, int c,
                                     const float *R, int64_t n_rel,
                                     const float *S, int64_t n_sub,
                                     const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                                     const float *dv, float *g_core, float *g_R, float *g_S,
                                     void *workspace, size_t workspace_bytes, void *stream);
int rtk_query_vectors_bwd_stream_bf16(const void *core, int a, int b, int c,
                                      const void *R, int64_t n_rel,
                                      const void *S, int64_t n_sub,
                                      const int64_t *rel_idx, const int64_t *sub_idx, int64_t batch,
                                      const float *dv, float *g_core, float *g_R, float *g_S,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* Backward of the logistic (R_TuckER.py:48): dZ = dP * P * (1 - P), n contiguous elements. */
int rtk_sigmoid_grad_f32(const float *dP, const float *P, float *dZ, int64_t n, void *stream);

/* the same with a row pitch (in elements) per array: dZ on 128-byte aligned rows for the GEMMs */
int rtk_sigmoid_grad_rows_f32(const float *dP, int64_t ld_dp, const float *P, int64_t ld_p, float *dZ,
                              int64_t ld_dz, int64_t batch, int64_t n, void *stream);

/*
 * Filtered rank of the queried object, on the device -- replaces the full B x N sort of the
 * eval tail (train.py:115-117; src/utils/utils.py:15-22 filter_predictions + src/utils/metrics.py:5-8).
 *   P          (batch x ld) scores, as written by the score stage (not modified)
 *   obj_idx    queried object id per row (features[:, 2])
 *   pair_slot  per row, index into the CSR of known-true objects of its (subject, relation)
 *              pair, or NULL for "no filtering"; pair_ptr / pair_obj: that CSR (int64)
 *   ranks_out  int32: 1 + #{j: p'_j > p_t} + #{j < t: p'_j == p_t}, p' = scores with the other
 *              true objects set to 0  (= position in a stable descending sort)
 *   bce_rows_out  optional double[batch]: per-row sum of nn.BCELoss terms against the 0/1 targets
 *              (train.py:113), logs clamped at -100 like torch; NULL to skip
 */
int rtk_filtered_rank_f32(const float *P, int64_t batch, int64_t n_ent, int64_t ld,
                          const int64_t *obj_idx, const int64_t *pair_slot,
                          const int64_t *pair_ptr, const int64_t *pair_obj,
                          int32_t *ranks_out, double *bce_rows_out, void *stream);

/*
 * Batch sums of the metrics (src/utils/metrics.py:4-22: mrr = sum 1/rank, hits@k = #(rank <= k)) and of
 * the BCE row sums, ADDED to acc5[0..4] = (sum 1/rank, hits@1, hits@3, hits@10, bce) -- the running
 * totals train.py:118-121 keeps per evaluation, without a device -> host copy per batch.
 */
int rtk_rank_metrics_f64(const int32_t *ranks, const double *bce_rows, int64_t batch, double *acc5, void *stream);
/* The same with every BCE row sum multiplied by bce_scale first: the reference averages the per-batch MEAN losses
 * (train.py:113,125), i.e. bce_scale = 1 / (batch * n_ent), without a pass over the row sums in between. */
int rtk_rank_metrics_scaled_f64(const int32_t *ranks, const double *bce_rows, int64_t batch, double bce_scale,
                                double *acc5, void *stream);

/*
 * Kernel timer: the duration of ONE score-kernel launch as the device saw it -- begin and end of the kernel itself, the
 * figure a rocprofv3 kernel trace reports -- without a profiler.  (A pair of events recorded on the stream around a
 * launch also carries the event records' own stream time and the dispatch gap in front of the kernel: 2.5-3 us of a
 * 31 us kernel.)  rtk_timer_arm(t): the NEXT score kernel this thread launches through rtk_score_packed_* /
 * rtk_score_1vN_* (the column-group, wave-specialised and bf16 kernels; not the v3 split kernel or the exact-fp32 GEMM: there the timer reports an error) is launched
 * with the timer's two events (hipExtLaunchKernelGGL); rtk_timer_elapsed_ms waits for that kernel and returns its
 * duration.  Arming is per thread and consumed by one launch -- arm it directly in front of the stage-2 call
 * (rtk_score_packed_*): with bf16 operands and a relation rank above 32 stage 1 builds its tables on the same bf16
 * kernel and would take the timer.  bench.py's roofline.kernel_ms.
 */
int rtk_timer_create(void **timer);
int rtk_timer_arm(void *timer);
int rtk_timer_elapsed_ms(void *timer, float *ms);
int rtk_timer_destroy(void *timer);

/*
 * Training forward with the loss fused into the score kernel's epilogue (reference train.py:79,136:
 * nn.BCELoss(mean) of sigmoid scores against label-smoothed targets y = (1 - eps) multi_hot + eps / N,
 * src/data/Dataset.py:51-52).  fp32 operands, c <= 512, packed query planes from rtk_query_vectors_f32.
 *   rtk_score_packed_bce_f32: x_out[d, j] = p - eps / N  (0 where the fp32 score saturated to 1.0f / 0.0f: the
 *       reference's autograd gives a zero logit gradient there) = d BCE / d logit of a NEGATIVE entry, up to the
 *       factor g / (B N); partials_out[0 .. rtk_score_bce_partials()) receive per-workgroup sums of the entries' BCE
 *       terms taken as negatives (unused slots are zeroed).  The B x N matrix is written once, never re-read.
 *   rtk_bce_patch_pos_f32: the known objects of every pair (CSR, as rtk_bce_rows_f32): x <- x - (1 - eps), and
 *       rows_pos_out[4 d .. 4 d + 3] = four partial sums of the correction of row d's BCE sum (4 * batch doubles); the positives' logits are recomputed from the fp32
 *       query vectors v (B, c) and entity rows O (N, c) (x = p - eps / N cannot give back a p far below eps / N).
 *   loss = (sum(partials) + sum(rows_pos)) / (B N);   d loss / d logits = x * g / (B N).
 */
int rtk_score_bce_partials(void);
int rtk_score_packed_bce_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_local,
                             float *x_out, int64_t ld_out, float label_smoothing, double *partials_out, void *stream);
int rtk_bce_patch_pos_f32(float *X, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                          const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing,
                          const float *v, const float *O, int c, double *rows_pos_out, void *stream);

/*
 * The exchange step of the entity-sharded path (BASELINE.json north_star: "RCCL all-gather of
 * per-shard scores over xGMI"): one process per GPU, rank p holds entity rows [p * n_loc, (p + 1) * n_loc) and
 * writes its (B, pitch) score block into slot p of a (world, B, pitch) buffer; rtk_allgather_scores completes the
 * buffer IN PLACE on every rank (ncclAllGather's in-place form, enqueued on `stream`).  RCCL is bound at run time
 * (the copy already in the process, else librccl.so of the ROCm install); without it these return
 * RTK_ERR_UNSUPPORTED.  rtk_comm_unique_id: 128 bytes for rank 0 to hand to its peers by the host's own means.
 * rtk_comm_init uses the calling thread's current device; one communicator per process and GPU.
 * No counterpart in the reference (single device): the Python mirror is r_tucker_amd.sharded.
 */
int rtk_comm_unique_id(void *id_out_128_bytes);
int rtk_comm_init(int rank, int world, const void *unique_id_128_bytes, void **comm_out);
int rtk_allgather_scores(void *comm, void *buf, size_t bytes_per_rank, void *stream);
int rtk_comm_destroy(void *comm);

/*
 * Batched small Cholesky-QR factor step, float64: for each of `batch` symmetric positive semidefinite k x k Gram
 * matrices S = W^T W (row-major, contiguous, k <= 256), with D = sqrt(diag S) if `equilibrate` (else I) and
 *     A = D^-1 S D^-1 + (shift_diag + shift_trace * trace(S)) I = L L^T,
 * the upper triangular  R = L^T D  and  X = D^-1 L^-T :  W X has orthonormal columns, W = (W X) R, and
 * X X^T = (S + shift)^-1 when not equilibrated.  One workgroup per matrix, one launch, no workspace, no host
 * synchronisation, no failure status: a pivot that cancelled below  max(1e-14 of its diagonal entry of A, shift / 2)
 * is floored there.  Only the lower triangle of S (diagonal included) is read.  trace(S) <= 0 or not a number, or a
 * value that is not finite on or below the diagonal, gives zero R and X for that matrix (its neighbours in the batch
 * are not affected).  Finite outputs are promised for positive semi-definite S plus rounding noise of the order of
 * the floor, NOT for an indefinite S: behind a floored pivot the entries grow by 1 / sqrt(floor) per further floored
 * column and overflow on a grossly indefinite matrix.  The Riemannian optimizer step orthonormalises and inverts the
 * core's Gram matrices with it (replaces tucker_riemopt's QR / SVD / solve calls reached from
 * src/model/asymmetric/optim.py:86-89,107-108 and src/model/symmetric/optim.py:80-83,101-103).
 * Refused before anything is enqueued, outputs untouched: a null operand, batch outside [1, 2^20), two of the three
 * buffers equal, a negative shift (RTK_ERR_BAD_ARG); k outside [1, 256] (RTK_ERR_UNSUPPORTED).
 */
int rtk_gram_factor_f64(const void *S, int64_t batch, int k, int equilibrate, double shift_diag, double shift_trace,
                        void *R_out, void *X_out, void *stream);

/*
 * The same ranking with the entity dimension sharded over GPUs (no gather of the scores): a rank
 * holds columns [col0, col0 + n_local) of the score matrix; the count is a sum over columns.
 *   1. rtk_target_scores_f32: pt_out[d] = P[d, obj_idx[d] - col0] where this rank owns the queried
 *      object, -inf elsewhere;  all-reduce MAX over the ranks gives every rank the target scores;
 *   2. rtk_filtered_rank_partial_f32: counts_out[d] = this block's share of
 *      #{j: p'_j > p_t} + #{j < t: p'_j == p_t}  (obj_idx and pair_obj hold GLOBAL entity ids), and
 *      optionally its share of the row's BCE sum;  all-reduce SUM, then rank = 1 + count.
 * B x 12 bytes cross the links instead of B x N x 4 (train.py:113-117 on a sharded entity matrix).
 */
int rtk_target_scores_f32(const float *P, int64_t batch, int64_t n_local, int64_t ld, int64_t col0,
                          const int64_t *obj_idx, float *pt_out, void *stream);

int rtk_filtered_rank_partial_f32(const float *P, int64_t batch, int64_t n_local, int64_t ld, int64_t col0,
                                  const float *target_scores, const int64_t *obj_idx,
                                  const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                  int32_t *counts_out, double *bce_rows_out, void *stream);

/*
 * The two counts every tie-aware rank derives from, on a block of columns of the score matrix: the twin of
 * rtk_filtered_rank_partial_f32, with its arguments and argument checks.  For query d with object t = obj_idx[d] and
 * p' = the row with the query's other CSR objects set to 0 (the queried object is never counted, even when it is
 * listed; entries outside the block are skipped; the CSR lists each object once), over the block's columns
 * j = col0 + column:
 *   greater_out[d] = #{ j != t : p'_j >  target_scores[d] }
 *   equal_out[d]   = #{ j != t : p'_j == target_scores[d] }
 * both int32, IEEE comparisons: -0 == +0, a NaN never counts, a NaN target score gives 0 and 0.  The counts of the
 * blocks of any partition add up exactly (all-reduce SUM); the whole matrix is the block col0 = 0 with
 * rtk_target_scores_f32's scores.  The stable rank of rtk_filtered_rank_f32 is
 * 1 + greater + #{ j < t : p'_j == p_t }, so 1 + greater <= rank <= 1 + greater + equal, and
 *   optimistic = 1 + greater,   realistic = 1 + greater + equal / 2,   pessimistic = 1 + greater + equal.
 */
int rtk_filtered_tie_counts_partial_f32(const float *P, int64_t batch, int64_t n_local, int64_t ld, int64_t col0,
                                        const float *target_scores, const int64_t *obj_idx,
                                        const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                        int32_t *greater_out, int32_t *equal_out, void *stream);

/*
 * Batch sums of the metrics of the three tie-aware rank types, ADDED to acc13 (the running totals of an evaluation,
 * as rtk_rank_metrics_f64 keeps them for the stable rank):
 *   acc13[0..3]   optimistic  (sum 1/rank, hits@1, hits@3, hits@10),  rank = 1 + greater
 *   acc13[4..7]   realistic,                                          rank = 1 + greater + equal / 2
 *   acc13[8..11]  pessimistic,                                        rank = 1 + greater + equal
 *   acc13[12]     #(equal > 0): the queries whose rank the tie rule decides
 * One workgroup, a fixed order of additions (repeated calls give the same bits).  Null pointers and batch < 1 give
 * RTK_ERR_BAD_ARG.
 */
int rtk_tie_metrics_f64(const int32_t *greater, const int32_t *equal, int64_t batch, double *acc13, void *stream);

/*
 * Filtered top-k link prediction: the k best objects of every (subject, relation, ?) row, leaving out the objects
 * already known to be true -- what torch.topk on the score matrix cannot do (no exclusion list, no stable tie rule).
 *   P          (batch x ld) scores, f32 or bf16 (bf16 values compare as bf16); read, never written
 *   n_cols     candidates per row, ld >= n_cols
 *   col0       column j of P is entity col0 + j (an entity block or shard of the full row) ...
 *   col_ids    ... unless this (batch x ld_ids) int64 matrix is given ("merge mode", e.g. the concatenated top-k
 *              lists of several shards or blocks): column j of row d is entity col_ids[d * ld_ids + j]; an id < 0
 *              marks an absent candidate.  When a tie at the cut-off has to be split, merge mode takes the tied
 *              candidates in column order: concatenated best-first lists of ascending id ranges have equal values
 *              in ascending id order, so that is the id order
 *   pair_slot  per row, index into the CSR of known-true objects (pair_ptr / pair_obj, as rtk_filtered_rank_f32),
 *              or -1 for none; NULL: no filtering.  Those objects are REMOVED from the row (not set to 0 as
 *              filter_predictions does); ids outside this block are ignored
 *   keep_idx   optional, per row: an object never removed (-1 = none), e.g. the queried object
 *   k          1 <= k <= 1024, else RTK_ERR_BAD_ARG
 *   values_out (batch x k) float, ids_out (batch x k) int64: best first.  Descending by value; equal values by
 *              ascending id (torch.sort(descending=True, stable=True) and rtk_filtered_rank_f32's order).  -0.0 and
 *              +0.0 are equal (written as +0.0); every NaN ranks above +inf, NaNs tie with one another (written as
 *              one quiet NaN).  A row with fewer than k eligible candidates is padded with (-inf, -1).
 * Consistency with ranking: with keep_idx = obj_idx and a target score p_t > 0, rtk_filtered_rank_f32's rank r <= k
 * iff ids_out[d, r - 1] == obj_idx[d]; for r > k the object is not in the row.
 * One workgroup per row, deterministic; the workspace size is 0 at present (workspace may then be NULL).
 * Arguments are validated before anything touches the device.
 */
size_t rtk_select_topk_workspace_bytes(int64_t batch, int64_t n_cols, int k);
int rtk_select_topk_f32(const float *P, int64_t batch, int64_t n_cols, int64_t ld, int64_t col0,
                        const int64_t *col_ids, int64_t ld_ids, const int64_t *pair_slot, const int64_t *pair_ptr,
                        const int64_t *pair_obj, const int64_t *keep_idx, int k, float *values_out, int64_t *ids_out,
                        void *workspace, size_t workspace_bytes, void *stream);
int rtk_select_topk_bf16(const uint16_t *P, int64_t batch, int64_t n_cols, int64_t ld, int64_t col0,
                         const int64_t *col_ids, int64_t ld_ids, const int64_t *pair_slot, const int64_t *pair_ptr,
                         const int64_t *pair_obj, const int64_t *keep_idx, int k, float *values_out, int64_t *ids_out,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Candidate scoring: each query scores its own list of K entities instead of all N (triple scoring: K = 1;
 * sampled negatives; candidate-set evaluation).
 *   z[d, k] = v[d, :] . O[cand[d * ld_cand + k], :]        out[d * ld_out + k] = z, or its logistic
 *   v     (batch x c) fp32 query vectors (stage 1: rtk_query_vectors_*, or their v_out); c in [1, 1024]
 *   O     (n_ent x c) fp32 (_f32) or bf16 (_bf16, read as bf16); any c, any 4-byte-aligned O
 *   cand  int64, row d at cand + d * ld_cand; ld_cand == 0: one list of K ids shared by every query
 *   out   fp32 (batch x ld_out), ld_out >= K
 *   flags RTK_SCORE_SIGMOID, RTK_SCORE_SIGMOID_FAST with the meaning they have for rtk_score_packed_*
 *   workspace  the error word's holder: a 256-byte-aligned buffer of >= 256 bytes whose first word is the error
 *              word (the workspace of the stage 1 that made v serves)
 * Arithmetic: _bf16 rounds v to bf16 (v^) first, as rtk_score_packed_bf16; products are formed by fmaf (exact for
 * bf16 x bf16).  A wave holds the row: lane l takes the m elements j = i * W + l * w + q (w = 4 fp32 / 8 bf16,
 * W = 64 w, m = w * ceil(c / W)), sums them by an fmaf chain in (i, q) order, and the 64 lane sums are added by a
 * 6-level xor butterfly.  So  |z - v.o| <= gamma(m + 6) * sum_j |v_j||o_j|,  gamma(n) = n 2^-24 / (1 - n 2^-24)
 * (for _bf16 with v^ in place of v); m + 6 <= 22.
 * Determinism: that order depends on c alone.  The bits of z[d, k] depend only on v[d], O[e] and c -- not on k, K,
 * batch, ld_cand, ld_out, n_ent, or the other candidates of the wave: a triple scores the same in every list.
 * An id outside [0, n_ent) is clamped for the load, its entry is written as NaN and bit 1 of the error word is set.
 * Refused with RTK_ERR_BAD_ARG before anything is enqueued: null pointers, c < 1, batch < 0, K < 0, n_ent < 1,
 * ld_cand neither 0 nor >= K, ld_out < K, flags other than the two above, a workspace under 256 bytes or not
 * 256-byte aligned.  c > 1024 or batch x K >= 2^31: RTK_ERR_UNSUPPORTED.
 */
int rtk_score_candidates_f32(const float *v, int64_t batch, int c, const float *O, int64_t n_ent,
                             const int64_t *cand, int64_t ld_cand, int64_t k, float *out, int64_t ld_out,
                             unsigned flags, void *workspace, size_t workspace_bytes, void *stream);
int rtk_score_candidates_bf16(const float *v, int64_t batch, int c, const void *O, int64_t n_ent,
                              const int64_t *cand, int64_t ld_cand, int64_t k, float *out, int64_t ld_out,
                              unsigned flags, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of the candidate scores (of the logits z: apply the logistic's derivative first), dZ (batch x ld_dz):
 *   dv[d, :]  = sum_k dZ[d, k] O[cand[d, k], :]                 fp32 (batch x c); O read as fp32 or bf16
 *   gO[e, :]  = sum_{(d, k): cand[d, k] = e} dZ[d, k] v[d, :]    fp32 (n_ent x c), written in full (rows no
 *               candidate names are 0); v is the fp32 query vector (for _bf16 not rounded: the rule of the 1-vs-N
 *               backward)
 * Either output may be NULL.  Out-of-range candidates add nothing to either, whatever their dZ (NaN and inf
 * included).  No float atomics; two runs give the same bits.
 * dv: a quarter is ceil(K / 4) consecutive k -- quarter i holds the k in [i ceil(K / 4), min(K, (i + 1) ceil(K / 4))),
 * so trailing quarters may be empty (K = 5: 2, 2, 1, 0 entries).  Per element j each quarter starts from +0 and adds
 * fmaf(dZ[d, k], O[cand[d, k], j], q_i) in increasing k; then dv[d, j] = ((q0 + q1) + q2) + q3 by fp32 adds, an empty
 * quarter being +0.  So |dv - exact| <= gamma(ceil(K / 4) + 2) sum_k |dZ||o| per element.  The order depends on K
 * alone (not on batch, c, ld_dz, ld_cand or n_ent).  dv reads neither v (it must still be non-NULL: the argument rules)
 * nor the workspace: with gO == NULL, workspace may be NULL and workspace_bytes 0.  K == 0: dv is all +0.
 * gO orders the entries d K + k by entity on the device (stable radix sort: counts, offsets, a stable fill), sums
 * each entity's list in increasing d K + k in chunks (batch K / 4096 entries rounded up to 16, clamped to [16, 256]:
 * a function of batch K alone), and adds the chunk sums in chunk order.
 * The workspace (rtk_score_candidates_bwd_workspace_bytes, 256-byte aligned) is needed when gO is given.
 * Argument rules as the forward, and ld_dz >= K.
 */
size_t rtk_score_candidates_bwd_workspace_bytes(int64_t batch, int64_t k, int64_t n_ent);
int rtk_score_candidates_bwd_f32(const float *dz, int64_t ld_dz, const float *v, int64_t batch, int c,
                                 const float *O, int64_t n_ent, const int64_t *cand, int64_t ld_cand, int64_t k,
                                 float *dv, float *gO, void *workspace, size_t workspace_bytes, void *stream);
int rtk_score_candidates_bwd_bf16(const float *dz, int64_t ld_dz, const float *v, int64_t batch, int c,
                                  const void *O, int64_t n_ent, const int64_t *cand, int64_t ld_cand, int64_t k,
                                  float *dv, float *gO, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Training loss without dense targets (train.py:76-82 with criterion = nn.BCELoss, train.py:136;
 * targets as src/data/Dataset.py:43-53 builds them: y = (1 - eps) * multi_hot + eps / N).
 * The multi-hot part is the CSR of known objects per (subject, relation) pair (pair_slot per row;
 * every object of a pair listed once).
 *   rtk_bce_rows_f32  rows_out[d] = sum_j BCE(P[d,j], y[d,j])  (double; logs clamped at -100 like
 *                     torch); the reference's mean loss is sum(rows_out) / (batch * n_ent)
 *   rtk_bce_grad_f32  in place  P[d,j] <- (P[d,j] - y[d,j]) * grad_loss[0] * scale : with
 *                     scale = 1 / (batch * n_ent) this is d loss / d logits (P = sigmoid(logits)),
 *                     the left operand of the dO / dv GEMMs.  grad_loss is a DEVICE scalar.
 *                     Entries whose fp32 score is saturated (exactly 1.0f or 0.0f) become 0, as in the
 *                     reference's autograd (BCELoss backward x logistic backward = (p - y) * [p(1-p) / max(p(1-p), 1e-12)]).
 */
int rtk_bce_rows_f32(const float *P, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                     const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing,
                     double *rows_out, void *stream);

int rtk_bce_grad_f32(float *P, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                     const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing,
                     const float *grad_loss, float scale, void *stream);

/*
 * Filtered ranks without the (batch x n_ent) score matrix (rtk_score_rank.hip): the one-block call of the block form
 * below (col0 = 0, n_local = n_ent), on the caller's stream target_kernel (p_t of every query, kept in the workspace),
 * count_kernel, filter_kernel (only with pair_slot) and finish_kernel, which writes 1 + count.  For query d with object
 * t = obj_idx[d]
 *   rank[d] = 1 + #{ j : p'_j > p_t } + #{ j < t : p'_j == p_t }
 * on probabilities (the logistic RTK_SCORE_SIGMOID selects, with or without RTK_SCORE_SIGMOID_FAST; raw logits are not
 * ranked: flags without RTK_SCORE_SIGMOID give RTK_ERR_UNSUPPORTED), where p' is p with the query's other known-true
 * objects (pair_obj[pair_ptr[s] .. pair_ptr[s + 1]), s = pair_slot[d] >= 0) set to 0 -- the rule and tie rule of
 * rtk_filtered_rank_f32.  NaN never counts.  CSR entries outside [0, n_ent) are skipped.  pair_slot may be NULL.
 *   q_packed   packed query planes of the batch (stage 1, as for rtk_score_packed_*)
 *   bce_rows   NULL, or per-row BCE sums as rtk_filtered_rank_f32 returns them (every CSR object positive, logs
 *              clamped at -100); summation order differs, so they agree to ~1e-6 relative.  Reduced in the block
 *              form's fixed order (float partials per workgroup slot and query tile, added in slot order in float64;
 *              no float atomics): repeated calls give the same bits.
 *   workspace  rtk_score_rank_workspace_bytes (valid without a device), 256-byte aligned:
 *                  rtk_score_rank_part_workspace_bytes(dtype, batch, n_ent, c) + align256(4 * batch)
 *              -- the block layout at n_local = n_ent and the batch's p_t behind it (34.1 MB at batch 8192,
 *              n_ent 1 000 000; the query-stationary kernels this call ran on before needed 1.1 MB there).  Its first
 *              word is the error word (the workspace of the stage 1 that made q_packed serves, once large enough).
 * Exactness: each probability is computed with the element arithmetic of the stored kernels, so
 *   _f32:  ranks equal rtk_filtered_rank_f32 over the scores of rtk_score_packed_f32 with RTK_SCORE_KERNEL_WS and the
 *          same flags.  The default fp32 dispatch differs from those scores only on the column-group kernel's fifth-group
 *          columns (rtk_score_fifth_group_columns_f32; none outside 18 432 <= n_ent <= 40 960).
 *   _bf16: ranks equal rtk_filtered_rank_f32 over rtk_score_packed_bf16's fp32 scores.
 * A query's rank does not depend on its batch or its position in it.
 * Covered shapes: _f32 c <= 208, c % 4 == 0, 16-byte-aligned O (the ws kernel's); _bf16 c <= 512.  Others give
 * RTK_ERR_UNSUPPORTED.  Refused with RTK_ERR_BAD_ARG before anything is enqueued: null pointers, batch < 0,
 * n_ent < 1, c < 1, pair_slot without the CSR arrays, unknown flags, a workspace too small or not 256-byte aligned.
 * batch == 0 returns at once.  An object id outside [0, n_ent) sets bit 2 (value 4) of the error word (its rank is
 * taken against the clamped id).
 */
size_t rtk_score_rank_workspace_bytes(int dtype, int64_t batch, int64_t n_ent, int c);
int rtk_score_rank_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_ent,
                       const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                       const int64_t *pair_obj, unsigned flags, int32_t *ranks, double *bce_rows,
                       void *workspace, size_t ws_bytes, void *stream);
int rtk_score_rank_bf16(const void *q_packed, int64_t batch, int c, const void *O, int64_t n_ent,
                        const int64_t *obj_idx, const int64_t *pair_slot, const int64_t *pair_ptr,
                        const int64_t *pair_obj, unsigned flags, int32_t *ranks, double *bce_rows,
                        void *workspace, size_t ws_bytes, void *stream);

/*
 * The same ranking on one block of entity rows (an entity shard), without the (batch x n_local) score block
 * (rtk_score_rank.hip): the matrix-free twins of rtk_target_scores_f32 / rtk_filtered_rank_partial_f32.  The
 * caller holds rows [col0, col0 + n_local) of the (n_ent x c) entity matrix as O_local; obj_idx and pair_obj hold
 * GLOBAL entity ids.
 *   1. rtk_score_rank_targets_*: pt_out[d] = probability of (query d, obj_idx[d]) where the block owns the object
 *      (col0 <= obj_idx[d] < col0 + n_local, the id clamped into [0, n_ent) first), -inf elsewhere; all-reduce MAX
 *      over the ranks completes it.  An id outside [0, n_ent) sets bit 2 of the error word.
 *   2. rtk_score_rank_counts_*: counts_out[d] = this block's share of
 *      #{j : p'_j > pt[d]} + #{j < t : p'_j == pt[d]}, j = col0 + row, with the rule, tie rule and filter rule of
 *      rtk_score_rank_* (the query's other CSR objects count as probability 0, the queried object is never
 *      counted, NaN never counts, CSR entries outside the block are ignored; the CSR lists each object once);
 *      bce_rows_out (optional): its share of the row's BCE sum.  All-reduce SUM, then rank = 1 + count.
 * rtk_score_rank_* IS the one-block call (these two steps at col0 = 0, n_local = n_ent, the finish pass adding the
 * 1), so for one block 1 + counts equals its ranks by construction; for every other partition of [0, n_ent) into
 * blocks 1 + the sum of the blocks' counts EQUALS them too, in both logistic modes, because every probability has the
 * same bits in every block and integer counts add exactly.  pt after the MAX has the bits of that call's internal
 * target score.  The BCE shares sum to its bce_rows to ~1e-6 relative; they are reduced in a fixed order (no float
 * atomics): repeated calls give the same bits.
 * The dense pass of step 2 is entity-stationary: every row of O_local is converted into MFMA operands once per
 * call (once per query range when n_local < 65 536), not once per 32-query tile.
 * Workspace: rtk_score_rank_part_workspace_bytes (valid without a device), 256-byte aligned, for both steps:
 *     256 + 2 * align256(4 * S * batch) + 2 * align256(4 * 8 * batch),   S = min(512, ceil(n_local / 128)),
 * align256 rounding up to a multiple of 256: partial counts and BCE sums per resident workgroup (at most two per
 * CU) and per filter wave (8 per query); nothing grows with batch * n_local (34.1 MB at batch 8192,
 * n_local 125 000).  Its first word is the error word.
 * Covered shapes, flags and refusals as rtk_score_rank_*; in addition col0 < 0, n_local < 1 or
 * col0 + n_local > n_ent give RTK_ERR_BAD_ARG.  batch == 0 returns at once.
 */
size_t rtk_score_rank_part_workspace_bytes(int dtype, int64_t batch, int64_t n_local, int c);
int rtk_score_rank_targets_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                               int64_t col0, int64_t n_ent, const int64_t *obj_idx, unsigned flags, float *pt_out,
                               void *workspace, size_t ws_bytes, void *stream);
int rtk_score_rank_targets_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                int64_t col0, int64_t n_ent, const int64_t *obj_idx, unsigned flags, float *pt_out,
                                void *workspace, size_t ws_bytes, void *stream);
int rtk_score_rank_counts_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                              int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                              const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                              unsigned flags, int32_t *counts_out, double *bce_rows_out, void *workspace,
                              size_t ws_bytes, void *stream);
int rtk_score_rank_counts_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                               int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                               const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                               unsigned flags, int32_t *counts_out, double *bce_rows_out, void *workspace,
                               size_t ws_bytes, void *stream);

/*
 * The tie counts of rtk_filtered_tie_counts_partial_f32 on one block of entity rows without the (batch x n_local)
 * score block (rtk_score_rank.hip): step 2 of the block form above with the two counts in place of their stable
 * combination.  Arguments as rtk_score_rank_counts_*, pt the completed target scores of rtk_score_rank_targets_*:
 *   greater_out[d] = #{ j != t : p'_j >  pt[d] },   equal_out[d] = #{ j != t : p'_j == pt[d] },   j = col0 + row,
 * int32, with the filter rule of rtk_score_rank_counts_* (the query's other CSR objects count as probability 0, the
 * queried object is never counted, CSR entries outside the block are ignored) and IEEE comparisons (a NaN never
 * counts; a NaN pt gives 0 and 0).  Every probability has the bits it has in rtk_score_rank_counts_*, so over any
 * partition of [0, n_ent) into blocks the counts add up exactly to the whole range's, and
 * 1 + greater <= the rank of rtk_score_rank_* <= 1 + greater + equal.
 * The kernels are those of the counts in their tie form: the entity-stationary sweep packs both counts of a tile step
 * into one int (greater | equal << 16; neither passes 128 there) and unpacks them into two int32 partial planes, the
 * filter pass corrects both (an entry that becomes a 0 joins `equal` when pt is 0), the finish pass adds partials
 * and corrections in a fixed order; no atomics.
 * Workspace: rtk_score_rank_ties_workspace_bytes (valid without a device; 0 outside the covered range), 256-byte
 * aligned: the layout of rtk_score_rank_part_workspace_bytes, nothing grows with batch * n_local.  Its first word is
 * the error word (not written here).
 * Covered shapes, flags and refusals as rtk_score_rank_counts_*: RTK_SCORE_SIGMOID required; _f32 c <= 208,
 * c % 4 == 0, 16-byte-aligned O; _bf16 c <= 512.  Everything is refused before anything is enqueued; batch == 0
 * returns at once.
 */
size_t rtk_score_rank_ties_workspace_bytes(int dtype, int64_t batch, int64_t n_local, int c);
int rtk_score_rank_tie_counts_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                  int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                                  const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                  unsigned flags, int32_t *greater_out, int32_t *equal_out, void *workspace,
                                  size_t ws_bytes, void *stream);
int rtk_score_rank_tie_counts_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                   int64_t col0, int64_t n_ent, const float *pt, const int64_t *obj_idx,
                                   const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                                   unsigned flags, int32_t *greater_out, int32_t *equal_out, void *workspace,
                                   size_t ws_bytes, void *stream);

/*
 * Filtered top-k link prediction WITHOUT the (batch x n_ent) score matrix or a (batch x n_local) score block
 * (rtk_score_topk.hip): values_out / ids_out are exactly what rtk_select_topk_f32 writes for the block's probabilities
 * -- P (batch x n_local) of rtk_score_packed_f32 with RTK_SCORE_KERNEL_WS (_f32) or of rtk_score_packed_bf16's fp32
 * scores (_bf16) on rows [col0, col0 + n_local) of O, selected with col0, the same CSR, keep_idx and k: values bit for
 * bit, ids, the tie order (higher score, then lower id; -0 == +0; NaN above +inf), the (-inf, -1) padding.  The
 * element arithmetic is that of rtk_score_rank_* (the same fragments), so a probability has the same bits in every
 * block: the lists of any partition of [0, n_ent) into blocks, merged by rtk_select_topk_f32 in merge mode in
 * ascending block order, equal the whole range's list (col0 = 0, n_local = n_ent).
 * On the caller's stream, enqueue only (graph-capturable):
 *   1. the maximum probability of every (query, tile of 128 entity rows), entity-stationary (every row of O_local is
 *      converted into MFMA operands once per call, once per query range when n_local < 65 536);
 *   2. with pair_slot: the tiles that hold a filtered object of a query are scored again for that query and their
 *      maxima corrected to exclude the query's filtered objects;
 *   3. rtk_select_topk_f32 on the maxima: the k_t = min(k, ceil(n_local / 128)) best tiles per query;
 *   4. those tiles scored again, their 128 k_t probabilities and ids per query written in ascending id order;
 *   5. rtk_select_topk_f32 in merge mode on these candidates.
 * k tiles suffice: a tile left out is preceded by k tiles whose maxima are k distinct eligible objects, each ahead of
 * every object of that tile (a larger value, or an equal one with a lower id).
 *   q_packed   packed query planes of the batch (stage 1, as for rtk_score_packed_*)
 *   pair_slot, pair_ptr, pair_obj, keep_idx   as rtk_select_topk_f32 (GLOBAL ids; entries outside the block are
 *              ignored; an object listed twice is harmless); pair_slot and keep_idx may be NULL
 *   k          1 <= k <= 128, else RTK_ERR_BAD_ARG
 *   flags      RTK_SCORE_SIGMOID, optionally RTK_SCORE_SIGMOID_FAST: probabilities only (a masked row is -inf, which
 *              no probability is); without RTK_SCORE_SIGMOID: RTK_ERR_UNSUPPORTED
 *   workspace  rtk_score_topk_workspace_bytes (valid without a device; 0 for a k or c outside the covered range),
 *              256-byte aligned, with T = ceil(n_local / 128), k_t = min(k, T), align256 rounding up to 256:
 *                  256 + align256(4 batch T) + align256(4 batch k_t) + align256(8 batch k_t)
 *                      + align256(512 batch k_t) + align256(1024 batch k_t)
 *              -- only the first term grows with n_local, at 1/128 of the score block (256 MB at batch 8192,
 *              n_local 1 000 000); callers bound the rest by splitting the batch, which is exact.  Its first 256 bytes
 *              are the error word's header and are left alone.
 * Covered shapes: _f32 c <= 208, c % 4 == 0, 16-byte-aligned O; _bf16 c <= 512; batch < 2^24.  Others give
 * RTK_ERR_UNSUPPORTED.  Refused with RTK_ERR_BAD_ARG before anything is enqueued: null pointers, batch < 0, n_ent < 1,
 * c < 1, a block outside [0, n_ent), pair_slot without the CSR arrays, unknown flags, a workspace too small or not
 * 256-byte aligned.  batch == 0 returns at once.  Deterministic: one writer per value, no float atomics.
 */
size_t rtk_score_topk_workspace_bytes(int dtype, int64_t batch, int64_t n_local, int c, int k);
int rtk_score_topk_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local, int64_t col0,
                       int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                       const int64_t *keep_idx, int k, unsigned flags, float *values_out, int64_t *ids_out,
                       void *workspace, size_t ws_bytes, void *stream);
int rtk_score_topk_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local, int64_t col0,
                        int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                        const int64_t *keep_idx, int k, unsigned flags, float *values_out, int64_t *ids_out,
                        void *workspace, size_t ws_bytes, void *stream);

/*
 * The 1-vs-all BCE training loss and its gradients WITHOUT the (batch x n_ent) score matrix (rtk_bce_stream.hip): the
 * matrix-free form of rtk_score_packed_bce_f32 + rtk_bce_patch_pos_f32 and of the two batch x n_ent sized GEMMs of the
 * backward.  Same arithmetic: p = the ws score kernel's probability (Frag of rtk_score_rank_*, both logistic modes),
 * targets y = (1 - eps) * multi_hot + eps / n_ent with the multi-hot part given as the CSR (pair_slot[d] < 0: an empty
 * list; entries outside [0, n_ent) are skipped; every object of a pair once), logs clamped at -100, and the logit
 * gradient x = p - y, 0 where the fp32 p is exactly 1.0f or 0.0f.
 *   rtk_bce_stream_rows_f32    loss_rows_out[d] = sum_j BCE(p[d, j], y[d, j]) (float64; loss = sum / (batch n_ent)) and,
 *                              when dv_out is given, dv_out[d, :] = sum_j x[d, j] O[j, :] (batch x c, UNSCALED: multiply
 *                              by g / (batch n_ent) before rtk_query_vectors_bwd_f32).  dv_out NULL: the second tile
 *                              product is not computed.
 *   rtk_bce_stream_grad_o_f32  gO_out[j, :] = sum_d x[d, j] * scale[0] * v[d, :], all n_ent x c written (rows that no
 *                              term touches are 0).  v: the fp32 query vectors (batch x c); scale: one float on the
 *                              device (g / (batch n_ent)).
 * Both sweep all (query tile, entity tile) pairs once; the 32 x 32 tile of x is never stored but used as the operand
 * of the next MFMA: in sweep 1 (rows) the query is on the lane and the tile is the A operand of X O, in sweep 2
 * (grad_o) the entity is on the lane and the tile is the A operand of X^T V.  Both products are three f16 MFMAs per
 * k-step on hi/lo halves with fp32 accumulation (x scaled by 2^14; O and scale * v by the power of two that brings
 * their largest magnitude into [2^14, 2^15)).
 * Accuracy, per element against float64 of the fp32 operands (u = 2^-24, u22 = 2^-22; derivation and tests:
 * tests/golden/bce_stream_cases.py, tests/test_gpu_bce_stream_kernels.py).  A logit carries the split chain's error
 * dz <= (3 + 0.75 ceil(c / 16)) u22 sum_k |v_k| |O_jk|; its probability dp <= 1.01 p (1 - p) (darg + dz) + k u p with
 * darg = (2.25 |z| + 2) u, k = 3 (fast logistic) or (2.25 |z| + 6) u, k = 2 (exact): the roundings of 1 + e and of the
 * reciprocal are absolute errors of a number near 1, so ln(1 - p), formed from the fp32 p, is off by up to
 * -ln(1 - dp / (1 - p)) -- relative to 1 - p, not to p (at z = 15, 1 - p = 3.1e-7 and dp = 1.8e-7): the conditioning of
 * BCE on fp32 probabilities.  Saturated elements (p exactly 1.0f from z = 16.64 on, 0.0f below z = -88.7; between -89.5
 * and -86.5 the two logistics differ) are exact: x = 0 and the logs 0 and -100.
 *   loss_rows  per element t0 Lp + (1 - t0) Lq, Lp = -ln(1 - dp / p), Lq = -ln(1 - (dp + u (1 - p)) / (1 - p)), plus
 *              24 u of |t0 ln p| + |(1 - t0) ln(1 - p)| (rtk_clog at 4 u, the products, sixteen fp32 adds per lane and
 *              tile), float64 from there; a CSR entry adds (1 - eps) (Lp + Lq) and (ceil(n_d / 128) + 16) u of its |terms|.
 *   dv         sum_j (dp_j + u |x_j|) |O_jk| + (3 u22 + r_j u) sum_j |x_j| |O_jk| + 2^-39 (sum_j |O_jk| + max|O| sum_j |x_j|)
 *              + (32 ceil(n_d / 128) + 6) u (1 - eps) sum_t |O_tk| + 2 u |dv|, r_j <= 3 (16-row groups left in the split)
 *              + (splits left) + 2 the fp32 roundings a term passes; a query without an unsaturated element: zero bits.
 *   gO         the same with scale v for O (3 u22 + u: scale * v is rounded), the query groups for the entity groups
 *              and (m_j + 6) u for the m_j CSR entries the ordered scatter adds into row j; an entity that no
 *              unsaturated element touches: +0.0.
 * Summation orders (no float atomics; repeated calls give the same bits):
 *   rows:   a workgroup holds 128 queries and walks a contiguous range of 32-row entity tiles in increasing order; the
 *           entity tiles are cut into `splits` = max(1, 256 / ceil(batch / 128)) ranges -- a function of batch and the
 *           CU count only -- whose dv slabs and loss partials (one float sum per tile and lane, added in float64) are
 *           added in range order.  The positives are added last (per query: its CSR entries in four interleaved
 *           groups of 32, the groups in order).  A query's row of loss_rows and dv does not depend on the other
 *           queries of the batch or on its position within them (only on batch through `splits`).
 *   grad_o: a wave owns 32 rows of gO and adds the query tiles in increasing order onto the positives' share, which
 *           rtk_score_candidates_bwd's ordered scatter builds (stable sort by entity, fixed chunk order).
 * max_pos: an upper bound, known to the host, on the number of CSR entries of the batch's queries (a query counted
 * as often as it occurs); the ordered scatter's buffers have that size.  More entries than that set bit 3 (value 8) of
 * the error word and the surplus is dropped; below that the results do not depend on max_pos (the scatter's windows
 * have a fixed size).  rtk_bce_stream_rows_f32 needs no such bound (workspace for max_pos = 0).
 * Workspace: rtk_bce_stream_workspace_bytes(batch, n_ent, c, max_pos), valid without a device, 256-byte aligned; with
 * cp = 32 * ceil(c / 32), S = splits and align256 rounding up to a multiple of 256:
 *     512 + align256(8 S batch) + align256(32 batch) + align256(4 S batch cp) + 2 align256(4 batch c)
 *         + align256(128 cp ceil(batch / 32)) + align256(4 (batch + 1)) + 3 align256(4 max_pos)
 *         + the ordered scatter's buffers for max_pos entries (rtk_score_candidates_bwd_workspace_bytes(max_pos, 1, .)),
 * nothing of which grows with batch * n_ent (about 95 MB at batch 4096, c 200, max_pos 1 000 000, any n_ent).  Its
 * first word is the error word.
 * Covered shapes: fp32, c <= 208, c % 4 == 0, 16-byte-aligned O (the range of rtk_score_rank_f32); others give
 * RTK_ERR_UNSUPPORTED -- there is no fallback to the matrix form.  flags: RTK_SCORE_SIGMOID, optionally
 * RTK_SCORE_SIGMOID_FAST.  Refused with RTK_ERR_BAD_ARG before anything is enqueued: null pointers, negative sizes,
 * label smoothing outside [0, 1), unknown flags, a workspace too small or not 256-byte aligned.  batch == 0: rows
 * returns at once, grad_o zeroes gO_out.  Enqueue only on `stream`; graph-capturable.
 */
size_t rtk_bce_stream_workspace_bytes(int64_t batch, int64_t n_ent, int c, int64_t max_pos);
int rtk_bce_stream_rows_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_ent,
                            const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                            float label_smoothing, unsigned flags, double *loss_rows_out, float *dv_out,
                            void *workspace, size_t ws_bytes, void *stream);
int rtk_bce_stream_grad_o_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O,
                              int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                              const int64_t *pair_obj, int64_t max_pos, float label_smoothing, unsigned flags,
                              const float *scale, float *gO_out, void *workspace, size_t ws_bytes, void *stream);

/*
 * The same two sweeps on one block of entity rows (an entity shard): the caller holds rows [col0, col0 + n_local) of the
 * (n_ent x c) entity matrix as O_local; pair_obj holds GLOBAL entity ids (the conventions of rtk_score_rank_targets_* /
 * rtk_score_rank_counts_*).  The loss and dv are sums over entities and a row of gO belongs to the block that owns it:
 *   rtk_bce_stream_rows_part_f32    loss_rows_out[d] = the block's share of sum_j BCE(p[d, j], y[d, j]), j over the
 *                                   block's rows only; dv_out[d, :] = sum_{j in block} x[d, j] O[j, :] (unscaled; NULL:
 *                                   not computed).  All-reduce SUM over the ranks completes both (batch doubles in the
 *                                   forward, batch x c floats in the backward, before rtk_query_vectors_bwd_f32).
 *   rtk_bce_stream_grad_o_part_f32  gO_local_out (n_local x c) = the block's rows of gO, written in full; no exchange.
 * Summed (rows, dv) or concatenated (gO) over any partition of [0, n_ent) into blocks they are the outputs of
 * rtk_bce_stream_rows_f32 / rtk_bce_stream_grad_o_f32 on the whole matrix up to the order of the fp32 / fp64 sums
 * (per element within TWICE the whole-matrix bounds stated there: the fp32 sums run per block and then over the blocks,
 * and the power of two of O in the dv product is the block's own);
 * with col0 = 0 and n_local = n_ent they have those calls' bits (the whole-matrix entry points ARE this block).
 * The smoothing term is eps / n_ent, the GLOBAL entity count, and the caller's scale is g / (batch n_ent).  A CSR
 * entry e belongs to the block iff col0 <= e < col0 + n_local (local row e - col0); the others are skipped in the loss
 * correction, in the positives' share of dv and in the ordered scatter's lists (they keep their slot with the "adds
 * nothing" key, so the launch sequence depends on batch, c, n_local and max_pos only: static, graph-capturable).
 * max_pos bounds the CSR entries of the batch's queries in ALL blocks, as for the whole matrix.  The O-wide power of
 * two of sweep 1's second product comes from the block's own rows.  Element arithmetic, summation orders within the
 * block, determinism, flags, covered range and refusals as rtk_bce_stream_*; in addition col0 < 0, n_local < 1 or
 * col0 + n_local > n_ent give RTK_ERR_BAD_ARG before anything is enqueued.  batch == 0: rows returns at once, grad_o
 * zeroes gO_local_out.
 * Workspace: rtk_bce_stream_part_workspace_bytes(batch, n_local, c, max_pos), valid without a device, 256-byte
 * aligned, first word the error word; the formula of rtk_bce_stream_workspace_bytes,
 *     512 + align256(8 S batch) + align256(32 batch) + align256(4 S batch cp) + 2 align256(4 batch c)
 *         + align256(128 cp ceil(batch / 32)) + align256(4 (batch + 1)) + 3 align256(4 max_pos)
 *         + rtk_score_candidates_bwd_workspace_bytes(max_pos, 1, .),
 * cp = 32 * ceil(c / 32), S = max(1, 256 / ceil(batch / 128)): n_local does not enter, nothing grows with
 * batch * n_local.
 */
size_t rtk_bce_stream_part_workspace_bytes(int64_t batch, int64_t n_local, int c, int64_t max_pos);
int rtk_bce_stream_rows_part_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                 int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                 const int64_t *pair_obj, float label_smoothing, unsigned flags,
                                 double *loss_rows_out, float *dv_out, void *workspace, size_t ws_bytes, void *stream);
int rtk_bce_stream_grad_o_part_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O_local,
                                   int64_t n_local, int64_t col0, int64_t n_ent, const int64_t *pair_slot,
                                   const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos,
                                   float label_smoothing, unsigned flags, const float *scale, float *gO_local_out,
                                   void *workspace, size_t ws_bytes, void *stream);

/*
 * The block form on bf16 operands, object rank up to 512 (rtk_bce_stream_bf16.hip): rtk_bce_stream_rows_part_f32 /
 * rtk_bce_stream_grad_o_part_f32 with O_local in bf16 (n_local x c, no fp32 copy of it is made) and q_packed the bf16
 * planes of rtk_pack_query_vectors / rtk_query_vectors_bf16; loss_rows_out is float64, dv_out and gO_local_out are
 * float32.  The whole matrix is the block col0 = 0, n_local = n_ent.  Arithmetic:
 *   z = sum_k v^_k O_jk with v^ = the planes' bf16 rounding of v, the k-steps summed as rtk_score_packed_bf16 sums them
 *   (two interleaved chains at c <= 256, one above), so p has that kernel's bits, and those of rtk_score_rank_*_bf16
 *   and rtk_score_topk_bf16, in both logistic modes; x = p - y with y = (1 - eps) * multi_hot + eps / n_ent, n_ent the
 *   GLOBAL entity count (entries of other blocks are skipped), 0 where the fp32 p is exactly 1.0f or 0.0f; the logs of
 *   the BCE terms clamped at -100;
 *   dv = X O_local (unscaled);  gO_local = X^T (scale[0] * v) with the fp32 v passed to the call, NOT its bf16 rounding.
 * The second tile product of both sweeps is cut along the output columns: the 32-column tiles are dealt evenly to the
 * fewest chunks of at most four tiles (128 columns), one grid dimension; every chunk computes the score tile again
 * (about 1.75 x the MFMAs of an uncut sweep at c = 512, none extra at c <= 128) and one chunk forms the loss partials.
 * x enters both products as fp16 hi/lo at 2^14; O as ONE fp16 plane at the power of two that brings max |O_local| into
 * [2^14, 2^15) -- exact for a bf16 value above the fp16 subnormals -- and scale * v as fp16 hi/lo (two and three MFMAs
 * per k-step).  Accuracy per element against float64 of (v^, O, v): the bounds of rtk_bce_stream_* with the chain error
 * dz <= 2^-23 * 16 ceil(c / 16) sum_k |v^_k| |O_jk| (derivation and tests: tests/golden/bce_stream_bf16_cases.py,
 * tests/test_gpu_bce_stream_bf16_kernels.py); partitions at twice those bounds.  Summation orders, determinism (no
 * float atomics, a static launch sequence, repeated calls give the same bits), max_pos, the error word (bit 3: more
 * CSR entries than max_pos), flags, batch == 0 and dv_out == NULL as the fp32 forms; dv_out == NULL leaves the bits of
 * loss_rows_out unchanged.
 * Covered: c <= 512, c % 8 == 0 and a 16-byte-aligned O_local (the vector row path); anything else gives
 * RTK_ERR_UNSUPPORTED, the other refusals are the fp32 forms'.
 * Workspace: rtk_bce_stream_bf16_workspace_bytes(batch, n_local, c, max_pos), valid without a device, 0 for a shape
 * outside the covered range; the formula of rtk_bce_stream_part_workspace_bytes with cp = 32 * (the padded tile count
 * chunks * tiles per chunk), n_local does not enter.  rtk_bce_stream_workspace_bytes and
 * rtk_bce_stream_part_workspace_bytes keep their answers.
 */
size_t rtk_bce_stream_bf16_workspace_bytes(int64_t batch, int64_t n_local, int c, int64_t max_pos);
int rtk_bce_stream_rows_part_bf16(const void *q_packed, int64_t batch, int c, const void *O_local, int64_t n_local,
                                  int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                  const int64_t *pair_obj, float label_smoothing, unsigned flags,
                                  double *loss_rows_out, float *dv_out, void *workspace, size_t ws_bytes, void *stream);
int rtk_bce_stream_grad_o_part_bf16(const void *q_packed, const float *v, int64_t batch, int c, const void *O_local,
                                    int64_t n_local, int64_t col0, int64_t n_ent, const int64_t *pair_slot,
                                    const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos,
                                    float label_smoothing, unsigned flags, const float *scale, float *gO_local_out,
                                    void *workspace, size_t ws_bytes, void *stream);

/*
 * The 1-vs-all softmax cross-entropy training loss, the other standard loss of 1-vs-all link prediction: what a user
 * of the reference gets by replacing criterion = nn.BCELoss (train.py:76-82, :136) on sigmoid scores with
 * torch.nn.functional.cross_entropy on the logits, the targets of src/data/Dataset.py:43-53 normalised per row.  For
 * batch item d let P_d be the CSR list of its pair (every object once), n_d = |P_d|, N = n_ent, eps the smoothing:
 *     y[d, j]  = (1 - eps) [j in P_d] / n_d + eps / N          (first term absent when n_d = 0)
 *     w_d      = sum_j y[d, j] = (1 - eps) [n_d > 0] + eps
 *     lse_d    = log sum_j exp(z[d, j])                         (row maximum subtracted)
 *     loss     = (1 / B) sum_d ( w_d lse_d - sum_j y[d, j] z[d, j] )  = F.cross_entropy(z, y), mean reduction
 *     d loss / d z[d, j] = (w_d softmax(z_d)_j - y[d, j]) / B   (every column: there is no saturation rule)
 * pair_slot[d] < 0 is an empty list; entries outside [0, n_ent) are skipped.  n_d is the STORED list length
 * pair_ptr[s + 1] - pair_ptr[s]: a skipped entry adds no term but still counts in n_d (in 1 / n_d and in [n_d > 0]).
 *
 * Matrix form (rtk_ce.hip), on STORED fp32 logits Z (batch x n_ent, row pitch ld; any c -- what
 * rtk_score_*(flags without RTK_SCORE_SIGMOID) wrote):
 *   rtk_ce_rows_f32  one pass per row: lse_out[d] (float) and rows_out[d] = w_d lse_d - sum_j y z (float64
 *                    accumulation across groups of eight columns; loss = sum(rows_out) / batch)
 *   rtk_ce_grad_f32  in place  Z[d, j] <- (w_d exp(Z[d, j] - lse[d]) - y[d, j]) * grad_loss[0] * scale; with
 *                    scale = 1 / batch this is d loss / d logits, |.| <= |g| / batch, the left operand of the dO / dv
 *                    GEMMs.  grad_loss is a DEVICE scalar.
 */
int rtk_ce_rows_f32(const float *Z, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                    const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing, double *rows_out,
                    float *lse_out, void *stream);
int rtk_ce_grad_f32(float *Z, int64_t batch, int64_t n_ent, int64_t ld, const int64_t *pair_slot,
                    const int64_t *pair_ptr, const int64_t *pair_obj, float label_smoothing, const float *lse,
                    const float *grad_loss, float scale, void *stream);

/*
 * The same loss WITHOUT the (batch x n_ent) logit matrix (rtk_ce_stream.hip): the sweeps of rtk_bce_stream_* with the
 * softmax link.  z[d, j] is the accumulated value of the ws score kernel's split-fp16 chain times its row and column
 * factors, acc * srow * 2^-sh: the logit of rtk_score_rank_f32 / rtk_bce_stream_*, without the logistic.
 *   rtk_ce_stream_rows_f32  the forward, ONE sweep and no second tile product: every lane keeps an online (maximum, sum
 *                           of exp) and the sum of z of its query over its 16 entities per 32-row entity tile (columns
 *                           past n_ent: -inf for the lse, 0 for the sum); the partials of the `splits` entity ranges
 *                           are merged in range order in float64; the positives' term -(1 - eps) / n_d sum_{t in P_d} z_t
 *                           comes from re-scoring the CSR entries with the same chain.  loss_rows_out[d] (float64;
 *                           loss = sum / batch) and lse_out[d] (float).
 *   rtk_ce_stream_grad_f32  the backward, from lse: with x[d, j] = w_d exp(z[d, j] - lse[d]) - eps / N (|x| <= 1) and
 *                           the positives as the constant -(1 - eps) / n_d per CSR entry,
 *                             dv_out[d, :] = sum_j x[d, j] O[j, :]               (batch x c, UNSCALED: multiply by g / batch
 *                                                                              before rtk_query_vectors_bwd_f32), and
 *                             gO_out[j, :] = sum_d x[d, j] scale[0] v[d, :]      (all n_ent x c written; scale: one float
 *                                                                              on the device, g / batch).
 *                           Either output may be NULL: its sweep is skipped (v and scale are needed for gO_out only).
 * Tile products, summation orders, max_pos and the error word as rtk_bce_stream_*: sweep 1 cuts the entity tiles into
 * `splits` = max(1, 256 / ceil(batch / 128)) ranges, added in range order; sweep 2 adds the query tiles in increasing
 * order onto the positives' share from the ordered scatter; the tile's 32 values of lse and w travel with the query tile.
 * No float atomics, repeated calls give the same bits, nothing grows with batch * n_ent.  A row with w_d = 0 (eps = 0 and
 * an empty list) contributes nothing.
 * Workspace: rtk_ce_stream_workspace_bytes(batch, n_ent, c, max_pos) (rows: max_pos = 0), valid without a device,
 * 256-byte aligned, first word the error word; with cp = 32 * ceil(c / 32), S = splits:
 *     512 + align256(4 S batch) + 2 align256(8 S batch) + align256(32 batch) + align256(4 S batch cp)
 *         + 2 align256(4 batch c) + align256(128 cp ceil(batch / 32)) + align256(256 ceil(batch / 32))
 *         + align256(4 (batch + 1)) + 3 align256(4 max_pos) + rtk_score_candidates_bwd_workspace_bytes(max_pos, 1, .).
 * Covered shapes: fp32, c <= 208, c % 4 == 0, 16-byte-aligned O; others give RTK_ERR_UNSUPPORTED (no fallback to the
 * matrix form).  RTK_ERR_BAD_ARG before anything is enqueued: null pointers, negative sizes, label smoothing outside
 * [0, 1), a workspace too small or misaligned.  batch == 0: rows returns at once, grad zeroes gO_out.  Static launch
 * sequences on `stream`, no host synchronisation; graph-capturable.
 */
size_t rtk_ce_stream_workspace_bytes(int64_t batch, int64_t n_ent, int c, int64_t max_pos);
int rtk_ce_stream_rows_f32(const void *q_packed, int64_t batch, int c, const float *O, int64_t n_ent,
                           const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                           float label_smoothing, double *loss_rows_out, float *lse_out, void *workspace,
                           size_t ws_bytes, void *stream);
int rtk_ce_stream_grad_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O, int64_t n_ent,
                           const int64_t *pair_slot, const int64_t *pair_ptr, const int64_t *pair_obj,
                           int64_t max_pos, float label_smoothing, const float *lse, const float *scale,
                           float *dv_out, float *gO_out, void *workspace, size_t ws_bytes, void *stream);

/*
 * The same loss on one block of entity rows (an entity shard): the caller holds rows [col0, col0 + n_local) of the
 * (n_ent x c) entity matrix as O_local; pair_obj holds GLOBAL entity ids (the conventions of rtk_bce_stream_*_part_f32).
 * Unlike the BCE loss this one is NOT a sum over entities: the row's log-sum-exp couples the blocks.  So the forward
 * stops before the logarithm and the backward takes the lse of the WHOLE row from the caller:
 *   rtk_ce_stream_rows_part_f32  the block's partial state of every query d, j over the block's rows only:
 *                                  max_out[d]    = m = max_j z[d, j]                              (float)
 *                                  sumexp_out[d] = sum_j exp(z[d, j] - m)                         (float64, >= 1)
 *                                  lin_out[d]    = -t0 sum_j z[d, j]
 *                                                  - (1 - eps) / n_d sum_{t in P_d, t in block} z[d, t]   (float64)
 *                                with t0 = eps / n_ent, the GLOBAL entity count, and n_d the GLOBAL (stored) list
 *                                length.  The sweep and the positives are those of rtk_ce_stream_rows_f32; the
 *                                `splits` partials are merged in range order in float64 as there, without the
 *                                logarithm.  Over a partition of [0, n_ent) into blocks k the caller forms
 *                                  M = max_k m_k,  lse_d = M + log sum_k s_k exp(m_k - M)   (MAX, then SUM over ranks),
 *                                  loss_rows[d] = w_d lse_d + sum_k lin_k[d]                (SUM),
 *                                which is rtk_ce_stream_rows_f32's loss_rows_out up to the order of the float64 sums.
 *   rtk_ce_stream_grad_part_f32  rtk_ce_stream_grad_f32 on the block, given the GLOBAL lse (batch floats):
 *                                x[d, j] = w_d exp(z[d, j] - lse[d]) - eps / n_ent;
 *                                dv_out[d, :] = sum_{j in block} x[d, j] O_local[j, :] is the block's share (unscaled;
 *                                all-reduce SUM over the ranks completes it, batch x c floats, before
 *                                rtk_query_vectors_bwd_f32); gO_local_out (n_local x c) holds the block's rows of gO,
 *                                written in full, no exchange.  Either output may be NULL.
 * With col0 = 0 and n_local = n_ent, grad_part has the bits of rtk_ce_stream_grad_f32 (that entry point IS this block),
 * and max_out + log(sumexp_out), w lse + lin_out are rtk_ce_stream_rows_f32's lse and loss rows up to the last
 * rounding.  A CSR entry e belongs to the block iff col0 <= e < col0 + n_local (local row e - col0); the others are
 * skipped in lin_out, in the positives' share of dv and in the ordered scatter's lists, where they keep their slot
 * with the "adds nothing" key: the launch sequence depends on batch, c, n_local and max_pos only (static,
 * graph-capturable).  max_pos bounds the CSR entries of the batch's queries in ALL blocks.  The O-wide power of two of
 * the dv product comes from the block's own rows.  Element arithmetic, summation orders within the block, the error
 * word, covered range and refusals as rtk_ce_stream_*; in addition col0 < 0, n_local < 1 or col0 + n_local > n_ent
 * give RTK_ERR_BAD_ARG before anything is enqueued.  No float atomics; repeated calls give the same bits.
 * batch == 0: rows_part returns at once, grad_part zeroes gO_local_out.
 * Workspace: rtk_ce_stream_part_workspace_bytes(batch, n_local, c, max_pos) (rows_part: max_pos = 0), valid without a
 * device, 256-byte aligned, first word the error word; the formula of rtk_ce_stream_workspace_bytes: n_local does not
 * enter, nothing grows with batch * n_local.
 */
size_t rtk_ce_stream_part_workspace_bytes(int64_t batch, int64_t n_local, int c, int64_t max_pos);
int rtk_ce_stream_rows_part_f32(const void *q_packed, int64_t batch, int c, const float *O_local, int64_t n_local,
                                int64_t col0, int64_t n_ent, const int64_t *pair_slot, const int64_t *pair_ptr,
                                const int64_t *pair_obj, float label_smoothing, float *max_out, double *sumexp_out,
                                double *lin_out, void *workspace, size_t ws_bytes, void *stream);
int rtk_ce_stream_grad_part_f32(const void *q_packed, const float *v, int64_t batch, int c, const float *O_local,
                                int64_t n_local, int64_t col0, int64_t n_ent, const int64_t *pair_slot,
                                const int64_t *pair_ptr, const int64_t *pair_obj, int64_t max_pos, float label_smoothing,
                                const float *lse, const float *scale, float *dv_out, float *gO_local_out,
                                void *workspace, size_t ws_bytes, void *stream);

/*
 * Relation prediction (h, ?, t): the third mode of the trilinear form, with the model's own parameters.  For query d
 * with subject h_d and object t_d
 *     W[d, i, j] = sum_k G[i, j, k] * O[t_d, k]
 *     u[d, i]    = sum_j S[h_d, j] * W[d, i, j]        the "pair vector" (batch x a, fp32)
 *     z[d, r]    = sum_i u[d, i] * R[r, i]             the 1-vs-all logit of (h_d, r) at column t_d
 * rtk_pair_vectors_* computes u without writing W: the core's a*b rows take O's place in an entity-stationary sweep on
 * the packed planes of the gathered O[t_d] rows, each 32 x 32 tile of W is multiplied by S[h_d, j] in registers and
 * reduced over j; only batch * a * ceil(b / 32) partial sums reach the workspace (csrc/rtk_pair.hip).  Symmetric
 * model: pass E as S and O.  b and c need not be equal.
 *   u, ld_u   : fp32 (batch x a), row pitch ld_u >= a elements
 *   packed_u  : the packed planes of u for the operand type (what rtk_pack_query_vectors gives for u), size
 *               rtk_packed_query_bytes(dtype, batch, a); may be NULL; needs a <= 512
 * Stage 2 is an existing entry point: z = rtk_score_packed_*(packed_u, batch, a, R, n_rel, ...) with the flags that call
 * takes (fp32 with a % 4 != 0 runs on its v3 kernel), or rtk_score_f32(u, batch, a, R, n_rel, ...) for fp32 operands at
 * any a.  With bf16 operands the planes hold u ROUNDED to bf16 (nearest even), as the query vectors v are on the
 * 1-vs-all path; u itself stays fp32.
 * Arithmetic: _f32 is the split-fp16 arithmetic of rtk_score_packed_f32's ws kernel (O[t_d] packed as a query row, the
 * core's rows converted as entity rows, hi*hi + hi*lo + lo*hi per k-step, then acc * (row factor * column factor));
 * _bf16 forms exact bf16 products in rtk_score_packed_bf16's chains (O[t_d] is copied into the planes, not rounded).
 * S[h_d, j] enters as fp32; the b products of (d, i) are summed 32 at a time in a fixed tree and the ceil(b / 32) sums
 * in ascending order.  The bits of u[d, :] depend only on O[t_d], S[h_d], the core and the operand type -- not on
 * batch, on the query's place in it or on the other queries -- and repeated calls give the same bits (no atomics).
 * Ids are range-checked on device: an id outside is clamped and raises the workspace's error word (1: subject id,
 * 4: object id); the other rows of the batch are unaffected.
 * Covered: _f32 c <= 208, c % 4 == 0, 16-byte-aligned core; _bf16 c <= 512; any a, b >= 1 with a * 32 ceil(b / 32)
 * < 2^31 - 64; otherwise RTK_ERR_UNSUPPORTED ("c = .. above ..", "fp32 needs c % 4 == 0 and a 16-byte-aligned core").
 * Null operands, batch < 0, a size < 1, ld_u < a: RTK_ERR_BAD_ARG.  A workspace that is missing, smaller than
 * rtk_pair_vectors_workspace_bytes(dtype, batch, a, b, c) ("workspace of .. bytes given, .. needed") or not 256-byte
 * aligned: RTK_ERR_WORKSPACE.  All of these are reported without touching a device.  batch == 0 is a no-op (the index
 * vectors, u and the workspace may then be NULL).  The size query is valid without a device, 0 at batch <= 0 and for
 * shapes that are not covered, and grows with batch.
 */
size_t rtk_pair_vectors_workspace_bytes(int dtype, int64_t batch, int a, int b, int c);
int rtk_pair_vectors_f32(const float *core, int a, int b, int c, const float *S, int64_t n_subj, const float *O,
                         int64_t n_obj, const int64_t *subject_idx, const int64_t *object_idx, int64_t batch, float *u,
                         int64_t ld_u, void *packed_u, void *workspace, size_t ws_bytes, void *stream);
int rtk_pair_vectors_bf16(const void *core, int a, int b, int c, const void *S, int64_t n_subj, const void *O,
                          int64_t n_obj, const int64_t *subject_idx, const int64_t *object_idx, int64_t batch, float *u,
                          int64_t ld_u, void *packed_u, void *workspace, size_t ws_bytes, void *stream);

/*
 * Training relation prediction: the gradients of z[d, r] above (csrc/rtk_pair_bwd.hip).  Given dZ (batch x n_rel),
 *     du = dZ . R,   gR = dZ^T . u                          rtk_gemm_f32
 *     rS[d, j] = sum_i du[d, i] * sum_k G[i, j, k] O[t_d, k]     gS[e, :] = sum_{d: h_d = e} rS[d, :]
 *     rO[d, k] = sum_i du[d, i] * sum_j G[i, j, k] S[h_d, j]     gO[e, :] = sum_{d: t_d = e} rO[d, :]
 *     gG[i, j, k] = sum_d du[d, i] S[h_d, j] O[t_d, k]
 * Nothing of size batch x a*b is written.  fp32 only.
 *
 * rtk_pair_rows_f32:
 *     rows[d, j] = sum_i w[d, i] * sum_k core[i, j, k] X[x_idx[d], k]        (batch x b) fp32, row pitch ld_rows >= b
 * rS is this call on (core, O, t, du); rO is this call on the core with its last two axes transposed and (S, h, du).
 * It is rtk_pair_vectors_f32's sweep with i and j exchanged: the rows of the sweep are j * a_pad + i, a_pad =
 * 32 ceil(a / 32), a 32 x 32 tile of sum_k core[i, j, k] X[x_d, k] (the split-fp16 arithmetic of rtk_pair_vectors_f32)
 * is multiplied by w[d, i] (fp32, row pitch ld_w >= a) in registers, the a products of (d, j) are summed 32 at a time in
 * a fixed tree and the ceil(a / 32) sums in ascending order; only batch * b * ceil(a / 32) partial sums reach the
 * workspace.  The bits of rows[d, :] depend only on X[x_idx[d]], w[d, :] and the core; repeated calls give the same bits
 * (no atomics).  An id outside [0, n_x) is clamped and raises the workspace's error word (4); the other rows are
 * unaffected.  Covered shapes, refusals, return codes and messages as rtk_pair_vectors_f32: c <= 208, c % 4 == 0 and a
 * 16-byte-aligned core, b * 32 ceil(a / 32) < 2^31 - 64 ("dimension too large"): RTK_ERR_UNSUPPORTED; null operands,
 * batch < 0, a size < 1, ld_w < a, ld_rows < b: RTK_ERR_BAD_ARG; a workspace that is missing, smaller than
 * rtk_pair_rows_workspace_bytes(batch, a, b, c) or not 256-byte aligned: RTK_ERR_WORKSPACE.  batch == 0 is a no-op
 * after the shape checks.  The size query is valid without a device and 0 at batch <= 0 or a shape not covered.
 *
 * rtk_core_outer_f32:
 *     gG[i, j, k] = sum_d (x[d, i] * y[d, j]) * z[d, k]        (a, b, c) fp32, dense
 * by v_mfma_f32_32x32x2_f32.  The left operand element is the single fp32 product x[d, i] * y[d, j], formed while it is
 * staged and never written to memory.  ONE accumulation chain per output element, over d ascending from zero in k-tiles
 * of 16 (the last zero-padded), no split-K: the bits are those of rtk_gemm_f32 on the materialised X[d, i b + j] =
 * x[d, i] * y[d, j] (M-major X, lda = a*b; M-major z; M = a*b, N = c, K = batch).  batch == 0 zeroes gG.  Null operands,
 * a size < 1, batch < 0, a pitch below its width: RTK_ERR_BAD_ARG; a*b*c or batch outside 31 bits: RTK_ERR_UNSUPPORTED.
 *
 * rtk_scatter_rows_f32:
 *     out[e, :] = sum_{d: idx[d] = e} rows[d, :]        (n_out x n) fp32 dense; rows nobody names are zero
 * The ordered scatter with entity idx[d], owner d and factor 1, cut into windows of 256 sorted entries whatever the
 * batch: within an entity the rows are added in increasing d, each window's run from 0, a run over several windows as
 * the sum of the windows' partial sums in window order.  No float atomics.  Ids outside [0, n_out) add nothing.
 * n <= 1024 (RTK_ERR_UNSUPPORTED above), ld_rows >= n; workspace of rtk_scatter_rows_workspace_bytes(batch), 256-byte
 * aligned (RTK_ERR_WORKSPACE).  batch == 0 zeroes out.
 */
size_t rtk_pair_rows_workspace_bytes(int64_t batch, int a, int b, int c);
int rtk_pair_rows_f32(const float *core, int a, int b, int c, const float *X, int64_t n_x, const int64_t *x_idx,
                      const float *w, int64_t ld_w, int64_t batch, float *rows, int64_t ld_rows, void *workspace,
                      size_t ws_bytes, void *stream);
int rtk_core_outer_f32(const float *x, int64_t ld_x, int a, const float *y, int64_t ld_y, int b, const float *z,
                       int64_t ld_z, int c, int64_t batch, float *gG, void *stream);
size_t rtk_scatter_rows_workspace_bytes(int64_t batch);
int rtk_scatter_rows_f32(const int64_t *idx, const float *rows, int64_t ld_rows, int64_t batch, int n, int64_t n_out,
                         float *out, void *workspace, size_t ws_bytes, void *stream);

/*
 * The float64 Gram-type product of two tall fp32 blocks (csrc/rtk_tall_gram.hip): what the Cholesky-QR rounds of the
 * Riemannian step on a row-sharded factor put in front of their all-reduce (smalllinalg.tall_gram_f64_rows).
 *     C[i, j] = sum_{k < n} A[k, i] * B[k, j]        (p x q) float64, contiguous
 * A (n x p) and B (n x q) are fp32, row-major at row pitches lda >= p, ldb >= q (the column halves f[:, :k], f[:, k:]
 * of an n x 2k matrix are operands as they lie).  Every product is formed in float64, where it is exact; every sum is
 * accumulated in float64 by v_mfma_f64_16x16x4_f64; no float64 copy of an operand is written to memory.  The rows are
 * cut into a number of equal ranges (the last may be short) that depends on (n, p, q) only; within a range an element
 * is one chain over the rows in ascending order; the ranges' partial matrices go to the workspace and a second launch
 * adds them in range order.  No atomics: repeated calls give the same bits.  Always the same two launches, no host
 * synchronisation (capturable).  Non-finite values propagate.  Rows at or beyond n are never read, nor is anything
 * beyond column p / q of a row.  16-byte loads are used when both bases and pitches are 16-byte aligned and p % 4 ==
 * q % 4 == 0, element loads otherwise: the same sums in the same order.  A == B with equal pitch is allowed.
 * n == 0 writes zeros.
 * Covered: 1 <= p, q <= 1024 (RTK_ERR_UNSUPPORTED outside), any n >= 0.  Null operands or workspace, n < 0, a pitch
 * below its column count, a workspace smaller than rtk_tall_gram_f64_workspace_bytes(n, p, q) or not 256-byte aligned:
 * RTK_ERR_BAD_ARG.  All of these are reported before anything is enqueued; the outputs are untouched.  The size query
 * is valid without a device, a multiple of 256, 0 for n < 0 or a shape not covered, and at most 64 MiB: it is (number
 * of ranges) * p * q * 8 bytes and does not grow with n beyond the range count.
 */
size_t rtk_tall_gram_f64_workspace_bytes(int64_t n, int p, int q);
int rtk_tall_gram_f64(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t n, int p, int q, double *C,
                      void *workspace, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RTUCKER_HIP_H */
