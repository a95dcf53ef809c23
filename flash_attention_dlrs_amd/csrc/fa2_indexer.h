// Shared declarations of the MLA indexer (fa2_mla_indexer_logits, fa2_topk_indices, fa2_mla_indexer_topk, include/fa2_fwd.h): internal.
#pragma once
#include "fa2_common.h"

// One indexer problem as fa2_indexer_api.hip hands it over, arguments already checked.  Strides in elements of each tensor's dtype.
struct Fa2IndexerProblem {
    const void *Q;     // (B, H, N_q, d) in `dtype`
    const float *W;    // (B, H, N_q)
    const void *K;     // (B, S_k, d) or, with `table`, the pool (num_blocks, page_size, d), in `k_dtype`
    const float *KS;   // (B, S_k) or (num_blocks, page_size), or null = 1
    float *LG;         // (B, N_q, S_k)
    int64_t qs[4], ws[3], ks[3], kss[2], lgs[3];
    const int32_t *seqlens;  // device, B entries, or null (N_k = S_k)
    const int32_t *table;    // paged: entry [b, i] at b * table_stride + i, clamped to [0, num_blocks - 1] by the kernel that reads it
    int64_t table_stride;
    int32_t page_size, num_blocks;
    int32_t B, H, N_q, S_k, d;  // S_k: the capacity (max_blocks * page_size when paged)
    int32_t dtype, k_dtype, causal;
    // the selection (fa2_topk_indices): the score launchers do not read these
    int32_t topk;
    int32_t *idx;  // (B, N_q, topk)
    int64_t is[3];
    hipStream_t stream;
    // packed (ragged) queries (the _varlen entry points): cu_q non-null.  Q is (total_q, H, d), W (total_q, H), LG (total_q, S_k), idx
    // (total_q, topk), their strides in the fixed call's order with a batch stride of 0 -- {0, head, token, d}, {0, head, token},
    // {0, row, column}, {0, row, slot} -- so the packed row takes the query position's place in every address.  Sequence b owns
    // n_q(b) = fa2_varlen_seq(cu_q, b, total_q, max_q) rows from its start on, query i of them standing at N_k(b) - n_q(b) + i; N_q
    // holds max_q.  The packed instantiations of the three kernels, a translation unit each (fa2_indexer_mfma16_v.hip,
    // fa2_indexer_generic_v.hip, fa2_indexer_topk_v.hip).
    const int32_t *cu_q;
    int32_t total_q, max_q;
};

// n(b, qi): the candidate count of query qi of sequence b.  Position p = N_k(b) - N_q + qi; causal: keys 0 .. min(p, N_k(b) - 1), none
// for p < 0; else all N_k(b).  Non-decreasing in qi.
__device__ __forceinline__ int fa2_indexer_count(const int32_t *seqlens, int b, int S_k, int N_q, int qi, int causal) {
    int nk = seqlens ? seqlens[b] : S_k;
    nk = nk < 0 ? 0 : (nk > S_k ? S_k : nk);
    if (!causal) return nk;
    const int p = nk - N_q + qi;
    return p < 0 ? 0 : (p + 1 < nk ? p + 1 : nk);
}

// Matrix form (fa2_indexer_mfma16.hip, FA2_INDEXER_VARIANT_IDX16): 64 index heads of kIdxQB query positions against 64-key tiles.
constexpr int kIdxQB = 8;  // query positions per workgroup
bool fa2_indexer_mfma16_supports(const Fa2IndexerProblem &p);
int fa2_launch_indexer_mfma16(const Fa2IndexerProblem &p);
// VALU form (fa2_indexer_generic.hip, FA2_INDEXER_VARIANT_GENERIC): lane = key, a loop over the heads.
int fa2_launch_indexer_generic(const Fa2IndexerProblem &p);
// Selection (fa2_indexer_topk.hip): reads LG, lgs, seqlens, B, N_q, S_k, causal, topk, idx, is, stream.
int fa2_launch_topk_indices(const Fa2IndexerProblem &p);
// ... and their packed forms
bool fa2_indexer_mfma16_v_supports(const Fa2IndexerProblem &p);
int fa2_launch_indexer_mfma16_v(const Fa2IndexerProblem &p);
int fa2_launch_indexer_generic_v(const Fa2IndexerProblem &p);
int fa2_launch_topk_indices_v(const Fa2IndexerProblem &p);
// Split-row selection (fa2_indexer_topk_split.hip, packed: _v; fa2_topk_indices_split): `splits` >= 2 workgroups a row, each over
// `chunk` positions (a multiple of 1,024, splits * chunk >= S_k), rows <= 65,535; `workspace` 16-byte aligned, of
// fa2_topk_split_bytes(rows, splits) bytes with any contents.  The same fields of the problem as the selection above.
constexpr int kTopkBins0 = 2048, kTopkBins1 = 2048, kTopkBins2 = 1024, kTopkBins = kTopkBins0 + kTopkBins1 + kTopkBins2;
constexpr int kTopkMaxSplits = 256;
inline int64_t fa2_topk_split_bytes(int64_t rows, int splits) { return rows * (4 * (int64_t)kTopkBins + 8 * (int64_t)splits); }
int fa2_launch_topk_indices_split(const Fa2IndexerProblem &p, int splits, int chunk, void *workspace);
int fa2_launch_topk_indices_split_v(const Fa2IndexerProblem &p, int splits, int chunk, void *workspace);
// fp8 queries (the _q8 entry points, `dtype` and `k_dtype` both fp8).  Matrix form (fa2_indexer_mfma8.hip, FA2_INDEXER_VARIANT_IDX8):
// 64 index heads of kIdx8QB query positions against 64-key tiles on v_mfma_f32_16x16x128_f8f6f4, fixed and packed (_v); the VALU form's
// fp8-query instantiations (fa2_indexer_generic_q8.hip, _q8_v), in units of their own so the 16-bit units keep their code.
constexpr int kIdx8QB = 16;  // query positions per workgroup
bool fa2_indexer_mfma8_supports(const Fa2IndexerProblem &p);
int fa2_launch_indexer_mfma8(const Fa2IndexerProblem &p);
bool fa2_indexer_mfma8_v_supports(const Fa2IndexerProblem &p);
int fa2_launch_indexer_mfma8_v(const Fa2IndexerProblem &p);
int fa2_launch_indexer_generic_q8(const Fa2IndexerProblem &p);
int fa2_launch_indexer_generic_q8_v(const Fa2IndexerProblem &p);

// The indexer's front end (fa2_indexer_prep.hip; include/fa2_fwd.h fa2_mla_indexer_prepare_q, fa2_mla_indexer_append_rot and their
// packed forms): rotary, the 128-point Hadamard transform and the row quantisation of index queries and keys, one launch each.
// Query form: arguments already checked; strides in elements, the packed call's in the fixed call's order with a batch stride of 0 and
// N_q holding max_q, as Fa2IndexerProblem's.  It is the kernel's argument as well.
struct Fa2IndexerPrepProblem {
    const void *Q;    // (B, H, N_q, 128) in `dtype`, unit column stride
    const float *W;   // (B, H, N_q)
    void *QO;         // contiguous (B, H, N_q, 128) in `out_dtype`; packed: (total_q, H, 128)
    float *WO;        // contiguous (B, H, N_q); packed: (total_q, H)
    int64_t qs[3], ws[3];
    const int32_t *seqlens;  // read with tables only
    const void *cos, *sin;   // (S_rot, rotary_dim / 2) in `dtype`, unit last stride, or both null
    int64_t cos_stride, sin_stride;
    int32_t S_rot, rotary_dim, interleaved, hadamard;
    float weight_scale;
    int32_t B, H, N_q;
    int32_t dtype, out_dtype;
    const int32_t *cu_q;  // packed: non-null, with total_q and max_q
    int32_t total_q, max_q;
    hipStream_t stream;
};
int fa2_launch_indexer_prep_q(const Fa2IndexerPrepProblem &p);
// Key form: the index-key append's problem (fa2_decode.h; mode FA2_APPENDQ_IDX8 or _COPY, d = 128, 16-bit src with a unit column
// stride) with its rotary fields set or `hadamard`, the row transformed before it is stored.
struct Fa2AppendQProblem;
int fa2_launch_indexer_prep_k(const Fa2AppendQProblem &p, bool hadamard);
