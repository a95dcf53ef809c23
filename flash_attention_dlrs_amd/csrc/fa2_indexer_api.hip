// fa2_indexer_api.hip -- host side of the MLA indexer (include/fa2_fwd.h): fa2_mla_indexer_logits, fa2_topk_indices, fa2_mla_indexer_topk
// and fa2_mla_indexer_workspace_bytes, and their packed (_varlen) forms.  One call struct and one check order of its own, beside the attention calls' DecodeCall
// (fa2_decode_api.hip): every check runs before any launch, then the score kernel of the form the variant names -- AUTO: the matrix
// form where it runs, else the VALU form -- and the selection, on the call's stream.
#include "fa2_indexer.h"

namespace {

// The arguments as the entry points take them; `scores` / `select` say which halves the call has.
struct IndexerCall {
    bool scores, select;
    const void *q_idx;
    const float *weights;
    const void *k_idx;
    const float *k_scale;
    float *logits;
    const int64_t *q_strides, *w_strides, *k_strides, *k_scale_strides, *logit_strides;
    const int32_t *cache_seqlens, *block_table;
    int64_t block_table_stride;
    int32_t B, H_I, N_q, S_k, num_blocks, page_size, max_blocks, d_I, dtype_enum, k_dtype_enum, causal, variant;
    int32_t topk;
    int32_t *indices;
    const int64_t *index_strides;
    void *hip_stream;
    // the _varlen entry points: packed queries over cu_seqlens_q, every stride array already in the fixed call's order with a batch
    // stride of 0 (PackedStrides), N_q holding max_seqlen_q
    bool packed = false;
    const int32_t *cu_seqlens_q = nullptr;
    int32_t total_q = 0;
};

// The stride arrays of a packed call in the fixed call's order: {token, head, column} -> {0, head, token, column}, {token, head} ->
// {0, head, token}, {row, column} -> {0, row, column}; null stays null.
struct PackedStrides {
    int64_t q[4], w[3], lg[3], idx[3];
    const int64_t *q4(const int64_t *s) {
        if (!s) return nullptr;
        q[0] = 0; q[1] = s[1]; q[2] = s[0]; q[3] = s[2];
        return q;
    }
    const int64_t *w3(const int64_t *s) {
        if (!s) return nullptr;
        w[0] = 0; w[1] = s[1]; w[2] = s[0];
        return w;
    }
    static const int64_t *rows3(const int64_t *s, int64_t (&out)[3]) {
        if (!s) return nullptr;
        out[0] = 0; out[1] = s[0]; out[2] = s[1];
        return out;
    }
};

bool is_fp8(int32_t dt) { return dt == FA2_DTYPE_F8E4M3 || dt == FA2_DTYPE_F8E5M2; }

int bad(const char *fmt, const char *name) {
    fa2_set_error(fmt, name);
    return FA2_ERR_BAD_ARG;
}

int check_indexer(const IndexerCall &c, Fa2IndexerProblem &p) {
    const char *who = c.scores ? "mla indexer" : "topk indices";
    if (c.scores) {
        const void *ptrs[7] = {c.q_idx, c.weights, c.k_idx, c.q_strides, c.w_strides, c.k_strides, c.logits};
        const char *names[7] = {"q_idx", "weights", "k_idx", "q_strides", "w_strides", "k_strides", "logits"};
        for (int t = 0; t < 7; ++t)
            if (!ptrs[t]) return bad("mla indexer: null %s", names[t]);
        if (c.k_scale && !c.k_scale_strides) return bad("mla indexer: null %s with a non-null k_scale", "k_scale_strides");
    }
    if (!c.logits || !c.logit_strides) {
        fa2_set_error("%s: null %s", who, !c.logits ? "logits" : "logit_strides");
        return FA2_ERR_BAD_ARG;
    }
    if (c.select && (!c.indices || !c.index_strides)) {
        fa2_set_error("%s: null %s", who, !c.indices ? "indices" : "index_strides");
        return FA2_ERR_BAD_ARG;
    }
    if (c.scores) {
        for (int k = 0; k < 4; ++k)
            if (c.q_strides[k] < 0) return bad("mla indexer: negative strides are not supported (%s)", "q_strides");
        for (int k = 0; k < 3; ++k) {
            if (c.w_strides[k] < 0) return bad("mla indexer: negative strides are not supported (%s)", "w_strides");
            if (c.k_strides[k] < 0) return bad("mla indexer: negative strides are not supported (%s)", "k_strides");
        }
        if (c.k_scale && (c.k_scale_strides[0] < 0 || c.k_scale_strides[1] < 0))
            return bad("mla indexer: negative strides are not supported (%s)", "k_scale_strides");
    }
    for (int k = 0; k < 3; ++k) {
        if (c.logit_strides[k] < 0) {
            fa2_set_error("%s: negative strides are not supported (logit_strides)", who);
            return FA2_ERR_BAD_ARG;
        }
        if (c.select && c.index_strides[k] < 0) {
            fa2_set_error("%s: negative strides are not supported (index_strides)", who);
            return FA2_ERR_BAD_ARG;
        }
    }
    if (c.B < 1 || c.B > 65535) {
        fa2_set_error("%s: B must be in [1, 65535] (got %d)", who, c.B);
        return FA2_ERR_BAD_ARG;
    }
    if (c.scores && c.H_I < 1) {
        fa2_set_error("mla indexer: H_I must be >= 1 (got %d)", c.H_I);
        return FA2_ERR_BAD_ARG;
    }
    if (c.packed) {
        if (!c.cu_seqlens_q) {
            fa2_set_error("%s varlen: null cu_seqlens_q", who);
            return FA2_ERR_BAD_ARG;
        }
        if (c.total_q < 1 || c.total_q > (1 << 28)) {
            fa2_set_error("%s varlen: total_q must be in [1, 2^28] (got %d)", who, c.total_q);
            return FA2_ERR_BAD_ARG;
        }
        if (c.N_q < 1 || c.N_q > (1 << 28)) {
            fa2_set_error("%s varlen: max_seqlen_q must be in [1, 2^28] (got %d)", who, c.N_q);
            return FA2_ERR_BAD_ARG;
        }
    } else if (c.N_q < 1 || c.N_q > (1 << 28)) {
        fa2_set_error("%s: N_q must be in [1, 2^28] (got %d)", who, c.N_q);
        return FA2_ERR_BAD_ARG;
    }
    int64_t cap = c.S_k;
    const bool paged = c.scores && c.block_table;
    if (paged) {
        if (c.num_blocks < 1 || c.page_size < 1 || c.max_blocks < 1) {
            fa2_set_error("mla indexer: num_blocks, page_size and max_blocks must be >= 1 (got num_blocks=%d, page_size=%d, max_blocks=%d)",
                          c.num_blocks, c.page_size, c.max_blocks);
            return FA2_ERR_BAD_ARG;
        }
        cap = (int64_t)c.max_blocks * c.page_size;
        if (c.block_table_stride < 0) return bad("mla indexer: negative %s", "block_table_stride");
    }
    if (cap < 1 || cap > (1 << 28)) {
        fa2_set_error(paged ? "%s: the capacity max_blocks * page_size must be in [1, 2^28] (got %lld)" : "%s: S_k must be in [1, 2^28] (got %lld)",
                      who, (long long)cap);
        return FA2_ERR_BAD_ARG;
    }
    if (c.select && (c.topk < 1 || c.topk > (1 << 28))) {
        fa2_set_error("%s: topk must be in [1, 2^28] (got %d)", who, c.topk);
        return FA2_ERR_BAD_ARG;
    }
    if (c.scores) {
        if (c.dtype_enum != FA2_DTYPE_F16 && c.dtype_enum != FA2_DTYPE_BF16 && c.dtype_enum != FA2_DTYPE_F32) {
            fa2_set_error("mla indexer: dtype_enum %d (q_idx) must be FA2_DTYPE_F16, FA2_DTYPE_BF16 or FA2_DTYPE_F32", c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.k_dtype_enum != c.dtype_enum) {
            if (!is_fp8(c.k_dtype_enum)) {
                fa2_set_error("mla indexer: k_dtype_enum %d must be dtype_enum or FA2_DTYPE_F8E4M3 / FA2_DTYPE_F8E5M2", c.k_dtype_enum);
                return FA2_ERR_UNSUPPORTED;
            }
            if (c.dtype_enum == FA2_DTYPE_F32) {
                fa2_set_error("mla indexer: an fp8 k_idx (k_dtype_enum %d) goes with f16 / bf16 q_idx, not f32", c.k_dtype_enum);
                return FA2_ERR_UNSUPPORTED;
            }
            if (!c.k_scale) {
                fa2_set_error("mla indexer: null k_scale with an fp8 cache (k_dtype_enum %d)", c.k_dtype_enum);
                return FA2_ERR_BAD_ARG;
            }
        }
        if (c.d_I < 1 || c.d_I > 576) {
            fa2_set_error("mla indexer: d_I=%d must be in [1, 576]", c.d_I);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.variant != FA2_INDEXER_VARIANT_AUTO && c.variant != FA2_INDEXER_VARIANT_GENERIC && c.variant != FA2_INDEXER_VARIANT_IDX16) {
            fa2_set_error("mla indexer: unknown variant %d (auto 0, generic 1, idx16 2)", c.variant);
            return FA2_ERR_UNSUPPORTED;
        }
        // the largest grid a score form takes (the VALU form's: 256 keys of one position per workgroup)
        const long long gx = ((cap + 255) / 256) * (long long)c.N_q;
        if (gx > 0x7fffffffLL) {
            fa2_set_error("mla indexer: grid too large (key tiles * N_q = %lld)", gx);
            return FA2_ERR_BAD_ARG;
        }
    }
    if (c.select && !c.packed && (long long)c.B * c.N_q > 0x7fffffffLL) {  // (packed: total_q rows, <= 2^28)
        fa2_set_error("%s: grid too large (B * N_q = %lld)", who, (long long)c.B * c.N_q);
        return FA2_ERR_BAD_ARG;
    }

    p = Fa2IndexerProblem{};
    p.LG = c.logits;
    for (int k = 0; k < 3; ++k) p.lgs[k] = c.logit_strides[k];
    p.seqlens = c.cache_seqlens;
    p.B = c.B; p.N_q = c.N_q; p.S_k = (int32_t)cap; p.causal = c.causal != 0;
    p.stream = (hipStream_t)c.hip_stream;
    p.cu_q = c.packed ? c.cu_seqlens_q : nullptr;
    p.total_q = c.packed ? c.total_q : 0; p.max_q = c.packed ? c.N_q : 0;
    if (c.scores) {
        p.Q = c.q_idx; p.W = c.weights; p.K = c.k_idx; p.KS = c.k_scale;
        for (int k = 0; k < 4; ++k) p.qs[k] = c.q_strides[k];
        for (int k = 0; k < 3; ++k) { p.ws[k] = c.w_strides[k]; p.ks[k] = c.k_strides[k]; }
        for (int k = 0; k < 2; ++k) p.kss[k] = c.k_scale ? c.k_scale_strides[k] : 0;
        p.table = c.block_table;
        p.table_stride = paged ? c.block_table_stride : 0; p.page_size = paged ? c.page_size : 0; p.num_blocks = paged ? c.num_blocks : 0;
        p.H = c.H_I; p.d = c.d_I; p.dtype = c.dtype_enum; p.k_dtype = c.k_dtype_enum;
    }
    if (c.select) {
        p.topk = c.topk; p.idx = c.indices;
        for (int k = 0; k < 3; ++k) p.is[k] = c.index_strides[k];
    }
    return FA2_OK;
}

int run_indexer(const IndexerCall &c) {
    Fa2IndexerProblem p;
    int rc = check_indexer(c, p);
    if (rc != FA2_OK) return rc;
    if (c.scores) {
        const bool fits = c.packed ? fa2_indexer_mfma16_v_supports(p) : fa2_indexer_mfma16_supports(p);
        const bool matrix = c.variant == FA2_INDEXER_VARIANT_AUTO ? fits : c.variant == FA2_INDEXER_VARIANT_IDX16;
        // (a forced matrix form that cannot run: refused there)
        if (c.packed) rc = matrix ? fa2_launch_indexer_mfma16_v(p) : fa2_launch_indexer_generic_v(p);
        else rc = matrix ? fa2_launch_indexer_mfma16(p) : fa2_launch_indexer_generic(p);
        if (rc != FA2_OK) return rc;
    }
    if (!c.select) return FA2_OK;
    return c.packed ? fa2_launch_topk_indices_v(p) : fa2_launch_topk_indices(p);
}

}  // namespace

extern "C" {

int fa2_mla_indexer_logits(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                           const int64_t q_strides[4], const int64_t w_strides[3], const int64_t k_strides[3],
                           const int64_t k_scale_strides[2], const int64_t logit_strides[3], const int32_t *cache_seqlens,
                           const int32_t *block_table, int64_t block_table_stride, int32_t B, int32_t H_I, int32_t N_q, int32_t S_k,
                           int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum,
                           int32_t k_dtype_enum, int32_t causal, int32_t variant, void *hip_stream) {
    return run_indexer({true, false, q_idx, weights, k_idx, k_scale, logits, q_strides, w_strides, k_strides, k_scale_strides, logit_strides,
                        cache_seqlens, block_table, block_table_stride, B, H_I, N_q, S_k, num_blocks, page_size, max_blocks, d_I,
                        dtype_enum, k_dtype_enum, causal, variant, 0, nullptr, nullptr, hip_stream});
}

int fa2_topk_indices(const float *logits, const int64_t logit_strides[3], const int32_t *cache_seqlens, int32_t B, int32_t N_q,
                     int32_t S_k, int32_t topk, int32_t causal, int32_t *indices, const int64_t index_strides[3], void *hip_stream) {
    return run_indexer({false, true, nullptr, nullptr, nullptr, nullptr, const_cast<float *>(logits), nullptr, nullptr, nullptr, nullptr,
                        logit_strides, cache_seqlens, nullptr, 0, B, 0, N_q, S_k, 0, 0, 0, 0, 0, 0, causal, 0, topk, indices, index_strides,
                        hip_stream});
}

int fa2_mla_indexer_topk(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                         const int64_t q_strides[4], const int64_t w_strides[3], const int64_t k_strides[3],
                         const int64_t k_scale_strides[2], const int64_t logit_strides[3], const int32_t *cache_seqlens,
                         const int32_t *block_table, int64_t block_table_stride, int32_t B, int32_t H_I, int32_t N_q, int32_t S_k,
                         int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum,
                         int32_t causal, int32_t topk, int32_t *indices, const int64_t index_strides[3], int32_t variant,
                         void *hip_stream) {
    return run_indexer({true, true, q_idx, weights, k_idx, k_scale, logits, q_strides, w_strides, k_strides, k_scale_strides, logit_strides,
                        cache_seqlens, block_table, block_table_stride, B, H_I, N_q, S_k, num_blocks, page_size, max_blocks, d_I,
                        dtype_enum, k_dtype_enum, causal, variant, topk, indices, index_strides, hip_stream});
}

int64_t fa2_mla_indexer_workspace_bytes(int32_t B, int32_t N_q, int32_t S_k) {
    if (B < 1 || N_q < 1 || S_k < 1) return 0;
    const int64_t rows = (int64_t)B * N_q;  // < 2^47
    return rows > INT64_MAX / (4 * (int64_t)S_k) ? INT64_MAX : 4 * rows * S_k;
}

int fa2_mla_indexer_logits_varlen(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                                  const int64_t q_strides[3], const int64_t w_strides[2], const int64_t k_strides[3],
                                  const int64_t k_scale_strides[2], const int64_t logit_strides[2], const int32_t *cu_seqlens_q,
                                  const int32_t *cache_seqlens, const int32_t *block_table, int64_t block_table_stride, int32_t B,
                                  int32_t H_I, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size,
                                  int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum, int32_t causal,
                                  int32_t variant, void *hip_stream) {
    PackedStrides s;
    return run_indexer({true, false, q_idx, weights, k_idx, k_scale, logits, s.q4(q_strides), s.w3(w_strides), k_strides, k_scale_strides,
                        PackedStrides::rows3(logit_strides, s.lg), cache_seqlens, block_table, block_table_stride, B, H_I, max_seqlen_q,
                        S_k, num_blocks, page_size, max_blocks, d_I, dtype_enum, k_dtype_enum, causal, variant, 0, nullptr, nullptr,
                        hip_stream, true, cu_seqlens_q, total_q});
}

int fa2_topk_indices_varlen(const float *logits, const int64_t logit_strides[2], const int32_t *cu_seqlens_q,
                            const int32_t *cache_seqlens, int32_t B, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t topk,
                            int32_t causal, int32_t *indices, const int64_t index_strides[2], void *hip_stream) {
    PackedStrides s;
    return run_indexer({false, true, nullptr, nullptr, nullptr, nullptr, const_cast<float *>(logits), nullptr, nullptr, nullptr, nullptr,
                        PackedStrides::rows3(logit_strides, s.lg), cache_seqlens, nullptr, 0, B, 0, max_seqlen_q, S_k, 0, 0, 0, 0, 0, 0,
                        causal, 0, topk, indices, PackedStrides::rows3(index_strides, s.idx), hip_stream, true, cu_seqlens_q, total_q});
}

int fa2_mla_indexer_topk_varlen(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                                const int64_t q_strides[3], const int64_t w_strides[2], const int64_t k_strides[3],
                                const int64_t k_scale_strides[2], const int64_t logit_strides[2], const int32_t *cu_seqlens_q,
                                const int32_t *cache_seqlens, const int32_t *block_table, int64_t block_table_stride, int32_t B,
                                int32_t H_I, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size,
                                int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum, int32_t causal, int32_t topk,
                                int32_t *indices, const int64_t index_strides[2], int32_t variant, void *hip_stream) {
    PackedStrides s;
    return run_indexer({true, true, q_idx, weights, k_idx, k_scale, logits, s.q4(q_strides), s.w3(w_strides), k_strides, k_scale_strides,
                        PackedStrides::rows3(logit_strides, s.lg), cache_seqlens, block_table, block_table_stride, B, H_I, max_seqlen_q,
                        S_k, num_blocks, page_size, max_blocks, d_I, dtype_enum, k_dtype_enum, causal, variant, topk, indices,
                        PackedStrides::rows3(index_strides, s.idx), hip_stream, true, cu_seqlens_q, total_q});
}

int64_t fa2_mla_indexer_varlen_workspace_bytes(int32_t total_q, int32_t S_k) {
    if (total_q < 1 || S_k < 1) return 0;
    return 4 * (int64_t)total_q * S_k;  // < 2^64
}

}  // extern "C"
