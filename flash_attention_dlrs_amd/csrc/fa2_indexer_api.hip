// fa2_indexer_api.hip -- host side of the MLA indexer (include/fa2_fwd.h): fa2_mla_indexer_logits, fa2_topk_indices, fa2_mla_indexer_topk
// and fa2_mla_indexer_workspace_bytes, their packed (_varlen) forms and the fp8-query (_q8) forms of the four score-bearing calls.  One call struct and one check order of its own, beside the attention calls' DecodeCall
// (fa2_decode_api.hip): every check runs before any launch, then the score kernel of the form the variant names -- AUTO: the matrix
// form where it runs, else the VALU form -- and the selection, on the call's stream.  fa2_mla_indexer_append and _varlen, the write side of
// the index-key cache, are here too: their checks, then the quantising append kernel (fa2_decode_append_q.hip).  So is the indexer's front
// end -- fa2_mla_indexer_prepare_q, fa2_mla_indexer_append_rot and their packed forms: rotary, the Hadamard transform and the row
// quantisation of queries and keys (fa2_indexer_prep.hip).  And the selection with a row split over several workgroups
// (fa2_topk_indices_split, _varlen_split, fa2_topk_workspace_bytes, fa2_topk_num_splits; fa2_indexer_topk_split.hip).
#include "fa2_indexer.h"
#include "fa2_decode.h"

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
    // the _q8 entry points: fp8 q_idx AND k_idx, the variants AUTO / GENERIC / IDX8
    bool q8 = false;
    // the _split entry points of the selection: num_splits as the caller gave it (0: the heuristic) and the workspace
    bool split = false;
    int32_t num_splits = 1;
    void *workspace = nullptr;
    int64_t workspace_bytes = 0;
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
        if (c.q8) {
            if (!is_fp8(c.dtype_enum)) {
                fa2_set_error("mla indexer q8: dtype_enum %d (q_idx) must be FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2", c.dtype_enum);
                return FA2_ERR_UNSUPPORTED;
            }
            if (!is_fp8(c.k_dtype_enum)) {
                fa2_set_error("mla indexer q8: k_dtype_enum %d must be FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2", c.k_dtype_enum);
                return FA2_ERR_UNSUPPORTED;
            }
            if (!c.k_scale) {
                fa2_set_error("mla indexer: null k_scale with an fp8 cache (k_dtype_enum %d)", c.k_dtype_enum);
                return FA2_ERR_BAD_ARG;
            }
        } else if (c.dtype_enum != FA2_DTYPE_F16 && c.dtype_enum != FA2_DTYPE_BF16 && c.dtype_enum != FA2_DTYPE_F32) {
            fa2_set_error("mla indexer: dtype_enum %d (q_idx) must be FA2_DTYPE_F16, FA2_DTYPE_BF16 or FA2_DTYPE_F32", c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        } else if (c.k_dtype_enum != c.dtype_enum) {
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
        if (c.variant != FA2_INDEXER_VARIANT_AUTO && c.variant != FA2_INDEXER_VARIANT_GENERIC &&
            c.variant != (c.q8 ? FA2_INDEXER_VARIANT_IDX8 : FA2_INDEXER_VARIANT_IDX16)) {
            fa2_set_error(c.q8 ? "mla indexer q8: unknown variant %d (auto 0, generic 1, idx8 3)"
                               : "mla indexer: unknown variant %d (auto 0, generic 1, idx16 2)", c.variant);
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

// The split count and the chunk of a selection, after check_indexer: 1 for the one-workgroup kernel (every call but the _split entry
// points; there num_splits 1, a heuristic that says 1, and a row of one chunk).  Else the count clamped to the chunks of 1,024
// positions the capacity holds, the chunk ceil(S_k / count) rounded up to 1,024, and the count once more the chunks that hold a
// position; then the workspace's checks.
int resolve_splits(const IndexerCall &c, const Fa2IndexerProblem &p, int &splits, int &chunk) {
    splits = 1;
    chunk = 0;
    if (!c.split) return FA2_OK;
    if (c.num_splits < 0 || c.num_splits > kTopkMaxSplits) {
        fa2_set_error("topk indices: num_splits must be in [0, %d] (got %d)", kTopkMaxSplits, c.num_splits);
        return FA2_ERR_BAD_ARG;
    }
    const int64_t rows = c.packed ? (int64_t)c.total_q : (int64_t)c.B * c.N_q;
    int ns = c.num_splits ? c.num_splits : fa2_topk_num_splits(rows, p.S_k, p.topk);
    const int most = (p.S_k + 1023) / 1024;
    ns = ns < most ? ns : most;
    if (ns <= 1) return FA2_OK;
    const int ch = ((p.S_k + ns - 1) / ns + 1023) / 1024 * 1024;
    ns = (p.S_k + ch - 1) / ch;
    if (ns <= 1) return FA2_OK;
    if (!c.workspace || ((uintptr_t)c.workspace & 15) != 0) {
        fa2_set_error(!c.workspace ? "topk indices: null workspace with num_splits = %d" : "topk indices: workspace must be 16-byte aligned (num_splits = %d)", ns);
        return FA2_ERR_BAD_ARG;
    }
    if (c.workspace_bytes < fa2_topk_split_bytes(rows, ns)) {
        fa2_set_error("topk indices: workspace_bytes = %lld is short of the %lld bytes %lld rows at num_splits = %d need", (long long)c.workspace_bytes,
                      (long long)fa2_topk_split_bytes(rows, ns), (long long)rows, ns);
        return FA2_ERR_BAD_ARG;
    }
    if (rows > 65535) {
        fa2_set_error("topk indices: grid too large for num_splits = %d (rows = %lld, the split form takes 65535)", ns, (long long)rows);
        return FA2_ERR_BAD_ARG;
    }
    splits = ns;
    chunk = ch;
    return FA2_OK;
}

int run_indexer(const IndexerCall &c) {
    Fa2IndexerProblem p;
    int rc = check_indexer(c, p);
    if (rc != FA2_OK) return rc;
    int splits, chunk;
    rc = resolve_splits(c, p, splits, chunk);
    if (rc != FA2_OK) return rc;
    if (c.scores && c.q8) {  // fp8 queries: the forms of their own, chosen by the same rule
        const bool fits = c.packed ? fa2_indexer_mfma8_v_supports(p) : fa2_indexer_mfma8_supports(p);
        const bool matrix = c.variant == FA2_INDEXER_VARIANT_AUTO ? fits : c.variant == FA2_INDEXER_VARIANT_IDX8;
        if (c.packed) rc = matrix ? fa2_launch_indexer_mfma8_v(p) : fa2_launch_indexer_generic_q8_v(p);
        else rc = matrix ? fa2_launch_indexer_mfma8(p) : fa2_launch_indexer_generic_q8(p);
        if (rc != FA2_OK) return rc;
    } else if (c.scores) {
        const bool fits = c.packed ? fa2_indexer_mfma16_v_supports(p) : fa2_indexer_mfma16_supports(p);
        const bool matrix = c.variant == FA2_INDEXER_VARIANT_AUTO ? fits : c.variant == FA2_INDEXER_VARIANT_IDX16;
        // (a forced matrix form that cannot run: refused there)
        if (c.packed) rc = matrix ? fa2_launch_indexer_mfma16_v(p) : fa2_launch_indexer_generic_v(p);
        else rc = matrix ? fa2_launch_indexer_mfma16(p) : fa2_launch_indexer_generic(p);
        if (rc != FA2_OK) return rc;
    }
    if (!c.select) return FA2_OK;
    if (splits > 1) return c.packed ? fa2_launch_topk_indices_split_v(p, splits, chunk, c.workspace) : fa2_launch_topk_indices_split(p, splits, chunk, c.workspace);
    return c.packed ? fa2_launch_topk_indices_v(p) : fa2_launch_topk_indices(p);
}

// The arguments of fa2_mla_indexer_append; the packed call brings k_new_strides as {0, token, column} and N_new = 0.
struct IndexAppendCall {
    void *k_idx;
    const int64_t *k_strides;
    float *k_scale;
    const int64_t *k_scale_strides;
    const int32_t *block_table;
    int64_t block_table_stride;
    const void *k_new;
    const int64_t *k_new_strides;
    const int32_t *cache_seqlens;
    int32_t *seqlens_out;
    int32_t B, N_new, S_k, num_blocks, page_size, max_blocks, d_I, dtype_enum, k_dtype_enum;
    void *hip_stream;
    const int32_t *cu_seqlens_new = nullptr;  // packed: non-null
    int32_t total_new = 0, max_seqlen_new = 0;
    bool packed = false;
    // the _rot entry points: the row is rotated and transformed before it is stored (fa2_indexer_prep.hip)
    const void *rotary_cos = nullptr, *rotary_sin = nullptr;
    int64_t rotary_cos_stride = 0, rotary_sin_stride = 0;
    int32_t S_rot = 0, rotary_dim = 0, rotary_interleaved = 0, hadamard = 0;
};

// The rotary tables of the front end's calls: both or neither, rotary_dim even in [2, 128].
int check_prep_rotary(const char *who, const void *cos, const void *sin, int64_t cs, int64_t ss, int32_t S_rot, int32_t rd) {
    if ((cos == nullptr) != (sin == nullptr)) {
        fa2_set_error("%s: rotary_cos and rotary_sin go together (null %s)", who, cos ? "rotary_sin" : "rotary_cos");
        return FA2_ERR_BAD_ARG;
    }
    if (!cos) return FA2_OK;
    if (S_rot < 1 || rd < 2 || rd > 128 || rd % 2 != 0) {
        fa2_set_error("%s: S_rot must be >= 1 and rotary_dim even in [2, 128] (got S_rot=%d, rotary_dim=%d)", who, S_rot, rd);
        return FA2_ERR_BAD_ARG;
    }
    if (cs < 0 || ss < 0) {
        fa2_set_error("%s: negative strides are not supported (rotary_cos_stride, rotary_sin_stride)", who);
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

// What the front end's kernels take: rows of 128 columns in f16 / bf16 with a unit column stride.  `what`: the rows' argument.
int check_prep_rows(const char *who, const char *what, int32_t d_I, int32_t dtype_enum, int64_t col_stride) {
    if (d_I != 128) {
        fa2_set_error("%s: d_I=%d: rotary and the Hadamard transform take d_I = 128", who, d_I);
        return FA2_ERR_UNSUPPORTED;
    }
    if (dtype_enum != FA2_DTYPE_F16 && dtype_enum != FA2_DTYPE_BF16) {
        fa2_set_error("%s: dtype_enum %d (%s) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16 (f32 rows are not rotated or transformed)", who,
                      dtype_enum, what);
        return FA2_ERR_UNSUPPORTED;
    }
    if (col_stride != 1) {
        fa2_set_error("%s: %s needs a unit column stride (got %lld)", who, what, (long long)col_stride);
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

// Every check of the index-key append, before any launch; then the launch.
int run_index_append(const IndexAppendCall &c) {
    const char *who = "mla indexer append";
    const void *ptrs[6] = {c.k_idx, c.k_strides, c.k_new, c.k_new_strides, c.cache_seqlens, c.seqlens_out};
    const char *names[6] = {"k_idx", "k_strides", "k_new", "k_new_strides", "cache_seqlens", "seqlens_out"};
    for (int t = 0; t < 6; ++t)
        if (!ptrs[t]) return bad("mla indexer append: null %s", names[t]);
    if (c.seqlens_out == c.cache_seqlens) return bad("mla indexer append: %s must not be cache_seqlens (the call does not modify its lengths)", "seqlens_out");
    for (int k = 0; k < 3; ++k)
        if (c.k_strides[k] < 0 || c.k_new_strides[k] < 0) return bad("mla indexer append: negative strides are not supported (%s)", "k_strides, k_new_strides");
    if (c.B < 1 || c.B > 65535) {
        fa2_set_error("%s: B must be in [1, 65535] (got %d)", who, c.B);
        return FA2_ERR_BAD_ARG;
    }
    if (c.packed) {
        if (!c.cu_seqlens_new) return bad("mla indexer append varlen: null %s", "cu_seqlens_new");
        if (c.total_new < 1 || c.total_new > (1 << 28) || c.max_seqlen_new < 1 || c.max_seqlen_new > (1 << 28)) {
            fa2_set_error("%s varlen: total_new and max_seqlen_new must be in [1, 2^28] (got %d, %d)", who, c.total_new, c.max_seqlen_new);
            return FA2_ERR_BAD_ARG;
        }
    } else if (c.N_new < 1 || c.N_new > (1 << 28)) {
        fa2_set_error("%s: N_new must be in [1, 2^28] (got %d)", who, c.N_new);
        return FA2_ERR_BAD_ARG;
    }
    int64_t cap = c.S_k;
    if (c.block_table) {
        if (c.num_blocks < 1 || c.page_size < 1 || c.max_blocks < 1) {
            fa2_set_error("%s: num_blocks, page_size and max_blocks must be >= 1 (got num_blocks=%d, page_size=%d, max_blocks=%d)", who,
                          c.num_blocks, c.page_size, c.max_blocks);
            return FA2_ERR_BAD_ARG;
        }
        cap = (int64_t)c.max_blocks * c.page_size;
        if (c.block_table_stride < 0) return bad("mla indexer append: negative %s", "block_table_stride");
    }
    if (cap < 1 || cap > (1 << 28)) {
        fa2_set_error(c.block_table ? "%s: the capacity max_blocks * page_size must be in [1, 2^28] (got %lld)" : "%s: S_k must be in [1, 2^28] (got %lld)",
                      who, (long long)cap);
        return FA2_ERR_BAD_ARG;
    }
    if (c.dtype_enum != FA2_DTYPE_F16 && c.dtype_enum != FA2_DTYPE_BF16 && c.dtype_enum != FA2_DTYPE_F32) {
        fa2_set_error("%s: dtype_enum %d (k_new) must be FA2_DTYPE_F16, FA2_DTYPE_BF16 or FA2_DTYPE_F32", who, c.dtype_enum);
        return FA2_ERR_UNSUPPORTED;
    }
    const bool quant = c.k_dtype_enum != c.dtype_enum;
    if (quant) {
        if (!is_fp8(c.k_dtype_enum)) {
            fa2_set_error("%s: k_dtype_enum %d must be dtype_enum or FA2_DTYPE_F8E4M3 / FA2_DTYPE_F8E5M2", who, c.k_dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.dtype_enum == FA2_DTYPE_F32) {
            fa2_set_error("%s: an fp8 k_idx (k_dtype_enum %d) goes with f16 / bf16 k_new, not f32", who, c.k_dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
        if (!c.k_scale || !c.k_scale_strides) return bad("mla indexer append: null %s with an fp8 cache", !c.k_scale ? "k_scale" : "k_scale_strides");
        if (c.k_scale_strides[0] < 0 || c.k_scale_strides[1] < 0) return bad("mla indexer append: negative strides are not supported (%s)", "k_scale_strides");
    } else if (c.k_scale) {
        fa2_set_error("%s: k_scale goes with an fp8 cache (k_dtype_enum %d == dtype_enum)", who, c.k_dtype_enum);
        return FA2_ERR_BAD_ARG;
    }
    if (c.d_I < 1 || c.d_I > 576) {
        fa2_set_error("%s: d_I=%d must be in [1, 576]", who, c.d_I);
        return FA2_ERR_UNSUPPORTED;
    }
    if (int rc = check_prep_rotary(who, c.rotary_cos, c.rotary_sin, c.rotary_cos_stride, c.rotary_sin_stride, c.S_rot, c.rotary_dim)) return rc;
    const bool prep = c.rotary_cos || c.hadamard;
    if (prep)
        if (int rc = check_prep_rows(who, "k_new", c.d_I, c.dtype_enum, c.k_new_strides[2])) return rc;
    Fa2AppendQProblem q{};
    q.mode = quant ? FA2_APPENDQ_IDX8 : FA2_APPENDQ_COPY;
    q.cache = c.k_idx;
    q.cs[0] = c.k_strides[0]; q.cs[1] = 0; q.cs[2] = c.k_strides[1]; q.cds = c.k_strides[2];
    q.scale = quant ? c.k_scale : nullptr;
    for (int k = 0; k < 2; ++k) q.scs[k] = quant ? c.k_scale_strides[k] : 0;
    q.table = c.block_table;
    q.table_stride = c.block_table ? c.block_table_stride : 0;
    q.page_size = c.block_table ? c.page_size : 0; q.num_blocks = c.block_table ? c.num_blocks : 0;
    q.capacity = (int32_t)cap;
    q.src = c.k_new;
    q.sns[0] = c.k_new_strides[0]; q.sns[1] = 0; q.sns[2] = c.k_new_strides[1]; q.sns[3] = c.k_new_strides[2];
    q.seqlens = c.cache_seqlens; q.seqlens_out = c.seqlens_out;
    q.B = c.B; q.H_kv = 1; q.N_new = c.N_new; q.d = c.d_I;
    q.dtype = c.dtype_enum; q.cache_dtype = c.k_dtype_enum;
    q.cu_new = c.packed ? c.cu_seqlens_new : nullptr;
    q.total_new = c.packed ? c.total_new : 0; q.max_new = c.packed ? c.max_seqlen_new : 0;
    q.stream = (hipStream_t)c.hip_stream;
    if (!prep) return fa2_launch_decode_append_q(q);
    q.cos = c.rotary_cos; q.sin = c.rotary_sin;
    q.cos_stride = c.rotary_cos_stride; q.sin_stride = c.rotary_sin_stride;
    q.S_rot = c.S_rot; q.rotary_dim = c.rotary_cos ? c.rotary_dim : 0; q.interleaved = c.rotary_interleaved != 0;
    return fa2_launch_indexer_prep_k(q, c.hadamard != 0);
}

// The arguments of fa2_mla_indexer_prepare_q; the packed call brings its strides in the fixed call's order (PackedStrides) and N_q = 0.
struct PrepareQCall {
    const void *q_idx;
    const int64_t *q_strides;
    const float *weights;
    const int64_t *w_strides;
    void *q_out;
    float *weights_out;
    const int32_t *cache_seqlens;
    const void *rotary_cos, *rotary_sin;
    int64_t rotary_cos_stride, rotary_sin_stride;
    int32_t S_rot, rotary_dim, rotary_interleaved, hadamard;
    float weight_scale;
    int32_t B, H_I, N_q, d_I, dtype_enum, out_dtype_enum;
    void *hip_stream;
    const int32_t *cu_seqlens_q = nullptr;  // packed: non-null
    int32_t total_q = 0, max_seqlen_q = 0;
    bool packed = false;
};

// Every check of the query preparation, before any launch; then the launch.
int run_prepare_q(const PrepareQCall &c) {
    const char *who = c.packed ? "mla indexer prepare queries varlen" : "mla indexer prepare queries";
    const void *ptrs[6] = {c.q_idx, c.q_strides, c.weights, c.w_strides, c.q_out, c.weights_out};
    const char *names[6] = {"q_idx", "q_strides", "weights", "w_strides", "q_out", "weights_out"};
    for (int t = 0; t < 6; ++t)
        if (!ptrs[t]) {
            fa2_set_error("%s: null %s", who, names[t]);
            return FA2_ERR_BAD_ARG;
        }
    for (int k = 0; k < 4; ++k)
        if (c.q_strides[k] < 0 || (k < 3 && c.w_strides[k] < 0)) {
            fa2_set_error("%s: negative strides are not supported (q_strides, w_strides)", who);
            return FA2_ERR_BAD_ARG;
        }
    if (c.B < 1 || c.B > 65535 || c.H_I < 1 || c.H_I > 65536) {
        fa2_set_error("%s: B must be in [1, 65535] and H_I in [1, 65536] (got %d, %d)", who, c.B, c.H_I);
        return FA2_ERR_BAD_ARG;
    }
    if (c.packed) {
        if (!c.cu_seqlens_q) {
            fa2_set_error("%s: null cu_seqlens_q", who);
            return FA2_ERR_BAD_ARG;
        }
        if (c.total_q < 1 || c.total_q > (1 << 28) || c.max_seqlen_q < 1 || c.max_seqlen_q > (1 << 28)) {
            fa2_set_error("%s: total_q and max_seqlen_q must be in [1, 2^28] (got %d, %d)", who, c.total_q, c.max_seqlen_q);
            return FA2_ERR_BAD_ARG;
        }
    } else if (c.N_q < 1 || (int64_t)c.B * c.N_q > (1 << 28)) {
        fa2_set_error("%s: N_q must be >= 1 and B * N_q <= 2^28 (got B=%d, N_q=%d)", who, c.B, c.N_q);
        return FA2_ERR_BAD_ARG;
    }
    if (int rc = check_prep_rows(who, "q_idx", c.d_I, c.dtype_enum, c.q_strides[3])) return rc;
    if (c.out_dtype_enum != c.dtype_enum && !is_fp8(c.out_dtype_enum)) {
        fa2_set_error("%s: out_dtype_enum %d must be dtype_enum or FA2_DTYPE_F8E4M3 / FA2_DTYPE_F8E5M2", who, c.out_dtype_enum);
        return FA2_ERR_UNSUPPORTED;
    }
    if (int rc = check_prep_rotary(who, c.rotary_cos, c.rotary_sin, c.rotary_cos_stride, c.rotary_sin_stride, c.S_rot, c.rotary_dim)) return rc;
    if (c.rotary_cos && !c.cache_seqlens) {
        fa2_set_error("%s: null cache_seqlens with rotary tables (a query's position is counted from its sequence's length)", who);
        return FA2_ERR_BAD_ARG;
    }
    if (!(c.weight_scale - c.weight_scale == 0.0f)) {
        fa2_set_error("%s: weight_scale must be finite", who);
        return FA2_ERR_BAD_ARG;
    }
    if (((uintptr_t)c.q_out & 15) != 0) {
        fa2_set_error("%s: q_out must be 16-byte aligned", who);
        return FA2_ERR_BAD_ARG;
    }
    Fa2IndexerPrepProblem p{};
    p.Q = c.q_idx; p.W = c.weights; p.QO = c.q_out; p.WO = c.weights_out;
    for (int k = 0; k < 3; ++k) { p.qs[k] = c.q_strides[k]; p.ws[k] = c.w_strides[k]; }
    p.seqlens = c.cache_seqlens;
    p.cos = c.rotary_cos; p.sin = c.rotary_sin;
    p.cos_stride = c.rotary_cos_stride; p.sin_stride = c.rotary_sin_stride;
    p.S_rot = c.S_rot; p.rotary_dim = c.rotary_cos ? c.rotary_dim : 0; p.interleaved = c.rotary_interleaved != 0;
    p.hadamard = c.hadamard != 0;
    p.weight_scale = c.weight_scale;
    p.B = c.B; p.H = c.H_I; p.N_q = c.packed ? c.max_seqlen_q : c.N_q;
    p.dtype = c.dtype_enum; p.out_dtype = c.out_dtype_enum;
    p.cu_q = c.packed ? c.cu_seqlens_q : nullptr;
    p.total_q = c.packed ? c.total_q : 0; p.max_q = c.packed ? c.max_seqlen_q : 0;
    p.stream = (hipStream_t)c.hip_stream;
    return fa2_launch_indexer_prep_q(p);
}

}  // namespace

extern "C" {

int fa2_mla_indexer_append(void *k_idx, const int64_t k_strides[3], float *k_scale, const int64_t k_scale_strides[2],
                           const int32_t *block_table, int64_t block_table_stride, const void *k_new, const int64_t k_new_strides[3],
                           const int32_t *cache_seqlens, int32_t *seqlens_out, int32_t B, int32_t N_new, int32_t S_k, int32_t num_blocks,
                           int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum,
                           void *hip_stream) {
    return run_index_append({k_idx, k_strides, k_scale, k_scale_strides, block_table, block_table_stride, k_new, k_new_strides,
                             cache_seqlens, seqlens_out, B, N_new, S_k, num_blocks, page_size, max_blocks, d_I, dtype_enum, k_dtype_enum,
                             hip_stream});
}

int fa2_mla_indexer_append_varlen(void *k_idx, const int64_t k_strides[3], float *k_scale, const int64_t k_scale_strides[2],
                                  const int32_t *block_table, int64_t block_table_stride, const void *k_new,
                                  const int64_t k_new_strides[2], const int32_t *cu_seqlens_new, const int32_t *cache_seqlens,
                                  int32_t *seqlens_out, int32_t B, int32_t total_new, int32_t max_seqlen_new, int32_t S_k,
                                  int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum,
                                  int32_t k_dtype_enum, void *hip_stream) {
    int64_t ns[3];
    return run_index_append({k_idx, k_strides, k_scale, k_scale_strides, block_table, block_table_stride, k_new,
                             PackedStrides::rows3(k_new_strides, ns), cache_seqlens, seqlens_out, B, 0, S_k, num_blocks, page_size,
                             max_blocks, d_I, dtype_enum, k_dtype_enum, hip_stream, cu_seqlens_new, total_new, max_seqlen_new, true});
}

int fa2_mla_indexer_append_rot(void *k_idx, const int64_t k_strides[3], float *k_scale, const int64_t k_scale_strides[2],
                               const int32_t *block_table, int64_t block_table_stride, const void *k_new, const int64_t k_new_strides[3],
                               const int32_t *cache_seqlens, int32_t *seqlens_out, const void *rotary_cos, const void *rotary_sin,
                               int64_t rotary_cos_stride, int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim,
                               int32_t rotary_interleaved, int32_t hadamard, int32_t B, int32_t N_new, int32_t S_k, int32_t num_blocks,
                               int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum,
                               void *hip_stream) {
    return run_index_append({k_idx, k_strides, k_scale, k_scale_strides, block_table, block_table_stride, k_new, k_new_strides,
                             cache_seqlens, seqlens_out, B, N_new, S_k, num_blocks, page_size, max_blocks, d_I, dtype_enum, k_dtype_enum,
                             hip_stream, nullptr, 0, 0, false, rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot,
                             rotary_dim, rotary_interleaved, hadamard});
}

int fa2_mla_indexer_append_varlen_rot(void *k_idx, const int64_t k_strides[3], float *k_scale, const int64_t k_scale_strides[2],
                                      const int32_t *block_table, int64_t block_table_stride, const void *k_new,
                                      const int64_t k_new_strides[2], const int32_t *cu_seqlens_new, const int32_t *cache_seqlens,
                                      int32_t *seqlens_out, const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride,
                                      int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                                      int32_t hadamard, int32_t B, int32_t total_new, int32_t max_seqlen_new, int32_t S_k,
                                      int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum,
                                      int32_t k_dtype_enum, void *hip_stream) {
    int64_t ns[3];
    return run_index_append({k_idx, k_strides, k_scale, k_scale_strides, block_table, block_table_stride, k_new,
                             PackedStrides::rows3(k_new_strides, ns), cache_seqlens, seqlens_out, B, 0, S_k, num_blocks, page_size,
                             max_blocks, d_I, dtype_enum, k_dtype_enum, hip_stream, cu_seqlens_new, total_new, max_seqlen_new, true,
                             rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved,
                             hadamard});
}

int fa2_mla_indexer_prepare_q(const void *q_idx, const int64_t q_strides[4], const float *weights, const int64_t w_strides[3],
                              void *q_out, float *weights_out, const int32_t *cache_seqlens, const void *rotary_cos,
                              const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride, int32_t S_rot,
                              int32_t rotary_dim, int32_t rotary_interleaved, int32_t hadamard, float weight_scale, int32_t B,
                              int32_t H_I, int32_t N_q, int32_t d_I, int32_t dtype_enum, int32_t out_dtype_enum, void *hip_stream) {
    return run_prepare_q({q_idx, q_strides, weights, w_strides, q_out, weights_out, cache_seqlens, rotary_cos, rotary_sin,
                          rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, hadamard, weight_scale, B, H_I,
                          N_q, d_I, dtype_enum, out_dtype_enum, hip_stream});
}

int fa2_mla_indexer_prepare_q_varlen(const void *q_idx, const int64_t q_strides[3], const float *weights, const int64_t w_strides[2],
                                     void *q_out, float *weights_out, const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                                     const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride,
                                     int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                                     int32_t hadamard, float weight_scale, int32_t B, int32_t H_I, int32_t total_q,
                                     int32_t max_seqlen_q, int32_t d_I, int32_t dtype_enum, int32_t out_dtype_enum, void *hip_stream) {
    PackedStrides s;
    return run_prepare_q({q_idx, s.q4(q_strides), weights, s.w3(w_strides), q_out, weights_out, cache_seqlens, rotary_cos, rotary_sin,
                          rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, hadamard, weight_scale, B, H_I, 0,
                          d_I, dtype_enum, out_dtype_enum, hip_stream, cu_seqlens_q, total_q, max_seqlen_q, true});
}

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

// The selection with a row split over num_splits workgroups: the same argument lists through the same checks, then resolve_splits.
int fa2_topk_indices_split(const float *logits, const int64_t logit_strides[3], const int32_t *cache_seqlens, int32_t B, int32_t N_q,
                           int32_t S_k, int32_t topk, int32_t causal, int32_t *indices, const int64_t index_strides[3],
                           int32_t num_splits, void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return run_indexer({false, true, nullptr, nullptr, nullptr, nullptr, const_cast<float *>(logits), nullptr, nullptr, nullptr, nullptr,
                        logit_strides, cache_seqlens, nullptr, 0, B, 0, N_q, S_k, 0, 0, 0, 0, 0, 0, causal, 0, topk, indices, index_strides,
                        hip_stream, false, nullptr, 0, false, true, num_splits, workspace, workspace_bytes});
}

int fa2_topk_indices_varlen_split(const float *logits, const int64_t logit_strides[2], const int32_t *cu_seqlens_q,
                                  const int32_t *cache_seqlens, int32_t B, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                                  int32_t topk, int32_t causal, int32_t *indices, const int64_t index_strides[2], int32_t num_splits,
                                  void *workspace, int64_t workspace_bytes, void *hip_stream) {
    PackedStrides s;
    return run_indexer({false, true, nullptr, nullptr, nullptr, nullptr, const_cast<float *>(logits), nullptr, nullptr, nullptr, nullptr,
                        PackedStrides::rows3(logit_strides, s.lg), cache_seqlens, nullptr, 0, B, 0, max_seqlen_q, S_k, 0, 0, 0, 0, 0, 0,
                        causal, 0, topk, indices, PackedStrides::rows3(index_strides, s.idx), hip_stream, true, cu_seqlens_q, total_q,
                        false, true, num_splits, workspace, workspace_bytes});
}

int64_t fa2_topk_workspace_bytes(int64_t rows, int32_t num_splits) {
    if (rows < 1 || rows > (1LL << 31) || num_splits < 2 || num_splits > kTopkMaxSplits) return 0;
    return fa2_topk_split_bytes(rows, num_splits);
}

// The conservative form, not measured: split only below 256 rows (one row a CU keeps the chip busy without it), to about one chip
// wave of workgroups -- 256 CUs over the rows -- and never to chunks shorter than 1,024 positions.  1 below 8,192 keys: a condition.
int32_t fa2_topk_num_splits(int64_t rows, int32_t S_k, int32_t topk) {
    if (rows < 1 || rows >= 256 || S_k < 8192 || topk >= S_k) return 1;
    const int64_t want = (256 + rows - 1) / rows, most = ((int64_t)S_k + 1023) / 1024;  // want in [2, 256]
    return (int32_t)(want < most ? want : most);
}

// fp8 queries: the same argument lists through the same checks, `q8` set (include/fa2_fwd.h).
int fa2_mla_indexer_logits_q8(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                           const int64_t q_strides[4], const int64_t w_strides[3], const int64_t k_strides[3],
                           const int64_t k_scale_strides[2], const int64_t logit_strides[3], const int32_t *cache_seqlens,
                           const int32_t *block_table, int64_t block_table_stride, int32_t B, int32_t H_I, int32_t N_q, int32_t S_k,
                           int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum,
                           int32_t k_dtype_enum, int32_t causal, int32_t variant, void *hip_stream) {
    return run_indexer({true, false, q_idx, weights, k_idx, k_scale, logits, q_strides, w_strides, k_strides, k_scale_strides, logit_strides,
                        cache_seqlens, block_table, block_table_stride, B, H_I, N_q, S_k, num_blocks, page_size, max_blocks, d_I,
                        dtype_enum, k_dtype_enum, causal, variant, 0, nullptr, nullptr, hip_stream, false, nullptr, 0, true});
}

int fa2_mla_indexer_topk_q8(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                         const int64_t q_strides[4], const int64_t w_strides[3], const int64_t k_strides[3],
                         const int64_t k_scale_strides[2], const int64_t logit_strides[3], const int32_t *cache_seqlens,
                         const int32_t *block_table, int64_t block_table_stride, int32_t B, int32_t H_I, int32_t N_q, int32_t S_k,
                         int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum,
                         int32_t causal, int32_t topk, int32_t *indices, const int64_t index_strides[3], int32_t variant,
                         void *hip_stream) {
    return run_indexer({true, true, q_idx, weights, k_idx, k_scale, logits, q_strides, w_strides, k_strides, k_scale_strides, logit_strides,
                        cache_seqlens, block_table, block_table_stride, B, H_I, N_q, S_k, num_blocks, page_size, max_blocks, d_I,
                        dtype_enum, k_dtype_enum, causal, variant, topk, indices, index_strides, hip_stream, false, nullptr, 0, true});
}

int fa2_mla_indexer_logits_varlen_q8(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
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
                        hip_stream, true, cu_seqlens_q, total_q, true});
}

int fa2_mla_indexer_topk_varlen_q8(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
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
                        PackedStrides::rows3(index_strides, s.idx), hip_stream, true, cu_seqlens_q, total_q, true});
}

}  // extern "C"
