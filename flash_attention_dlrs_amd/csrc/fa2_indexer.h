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
