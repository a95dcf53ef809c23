// fa2_decode_api.hip -- extern "C" entry points of KV-cache decode attention (fa2_fwd_kvcache, _fp8, _paged, the latent-cache calls
// _mla, _mla_fp8, _mla_varlen and the key-list calls _mla_sparse and _mla_sparse_varlen, the packed-query call _varlen, the cache appends fa2_kvcache_append and _append_varlen, the fused steps
// fa2_fwd_kvcache_append, _varlen_append, _mla_append and _mla_varlen_append, and their helpers, declared in include/fa2_fwd.h).  Every attention call takes three steps:
//   1. fill   the entry point names its raw arguments in a DecodeCall (the cache update's in an AppendCall), packed strides through packed4;
//   2. check  check_decode (check_append) tests every argument, resolves num_splits (split_count on the unsplit workgroup count of the
//             call's form) and fills the Fa2DecodeProblem (Fa2AppendProblem); nothing is launched;
//   3. run    run_decode takes the call's row of kForms (fixed, packed, MLA, packed MLA) and launches, on the caller's stream, the append of a fused
//             step, the split kernel, then the combine.  A fused step runs all of check_append before any check of the attention.
#include "fa2_decode.h"

namespace {

// The split rule: enough splits to put `waves` x 256 workgroups on the chip, every split at least `min_tiles` key tiles long
// (judged on the capacity: the lengths live on the device).  `base` is the workgroup count of the unsplit launch of the form AUTO
// takes for the shape; the three heuristics below differ in how they count it and in the two constants.
constexpr int kChipWorkgroups = 256;  // one per CU
constexpr int64_t kMaxRows = 1LL << 40;  // B * H * N_q beyond this is refused: the workspace size stays far inside int64

int split_count(int64_t base, int64_t S_k, int waves, int min_tiles) {
    if (base >= kChipWorkgroups) return 1;
    int64_t n = (waves * kChipWorkgroups + base - 1) / base;
    const int64_t cap = (S_k + FA2_KVCACHE_KEY_TILE - 1) / FA2_KVCACHE_KEY_TILE / min_tiles;
    if (n > cap) n = cap;
    if (n > FA2_KVCACHE_MAX_SPLITS) n = FA2_KVCACHE_MAX_SPLITS;
    return n < 1 ? 1 : (int)n;
}

// The shape the heuristics judge: N_q is max_seqlen_q and total_q is read for packed queries only, d_v for the latent cache only.
struct SplitShape {
    int64_t B, H, H_kv, N_q, total_q, S_k;
    int32_t d, d_v, dtype;
};

// fa2_kvcache_num_splits: base = B * H_kv for the matrix form, B * H * ceil(N_q / 16) for the VALU form.  The constants are read
// off the num_splits sweep of benchmarks/bench_decode.py ("Decode attention").
constexpr int kSplitWaves = 2;
constexpr int kMinSplitTiles = 4;

int num_splits_auto(const SplitShape &s) {
    const bool mfma = fa2_decode_mfma16_shape((int32_t)s.H, (int32_t)s.H_kv, (int32_t)s.N_q, s.d, s.dtype);
    return split_count(mfma ? s.B * s.H_kv : s.B * s.H * ((s.N_q + 15) / 16), s.S_k, kSplitWaves, kMinSplitTiles);
}

// fa2_kvcache_mla_num_splits: the latent matrix form (fa2_decode_mla16.hip) runs ONE workgroup per CU (its LDS tile and registers
// fill it), base = B * H_kv * ceil(g N_q / 64) of them unsplit, so one wave of the chip is what the splits fill (kMlaSplitWaves),
// and a split is at least kMlaMinSplitTiles 64-key tiles long: each workgroup loads its 64 x 576 Q fragments and writes 64 x 512
// fp32 partials whatever its length.  The constants are read off the split sweep of benchmarks/bench_mla_decode.py (DESIGN.md,
// "MLA decode").  Every other shape is counted as the VALU form's.
constexpr int kMlaSplitWaves = 1;
constexpr int kMlaMinSplitTiles = 4;

int num_splits_mla(const SplitShape &s) {
    if (!fa2_decode_mla16_shape(s.d, s.d_v, s.dtype) || s.H_kv < 1 || s.H % s.H_kv != 0) {
        SplitShape valu = s;
        valu.d = 0;
        return num_splits_auto(valu);
    }
    return split_count(s.B * s.H_kv * ((s.H / s.H_kv * s.N_q + 63) / 64), s.S_k, kMlaSplitWaves, kMlaMinSplitTiles);
}

// fa2_kvcache_varlen_num_splits: base is the unsplit workgroup count of the packed launch.  A sequence fills ceil(n_q(b) / tq)
// query tiles, the lengths live on the device: the count is bounded by the grid, B * ceil(max_seqlen_q / tq), and by
// ceil(total_q / tq) + B (every sequence ends in at most one partly filled tile), per KV head of the matrix form
// (tq = min(64 / g, max_seqlen_q)), per query head of the VALU form (tq = 16).
int num_splits_varlen(const SplitShape &s) {
    const bool mfma = fa2_decode_mfma16_v_shape((int32_t)s.H, (int32_t)s.H_kv, s.d, s.dtype);
    const int64_t tq = mfma ? fa2_decode_varlen_tq((int32_t)(s.H / s.H_kv), (int32_t)s.N_q) : 16;
    const int64_t grid = s.B * ((s.N_q + tq - 1) / tq), packed = (s.total_q + tq - 1) / tq + s.B;
    return split_count((mfma ? s.H_kv : s.H) * (grid < packed ? grid : packed), s.S_k, kSplitWaves, kMinSplitTiles);
}

// fa2_kvcache_mla_varlen_num_splits: the packed bound above on the tile count of the query-tiled latent form
// (fa2_decode_mla16_v.hip): a sequence fills ceil(g n_q(b) / 64) row tiles per KV head, so the unsplit launch is at most the grid,
// B * ceil(g max_seqlen_q / 64), and at most ceil(g total_q / 64) + B.  One wave of the chip as for the fixed latent call, but a
// split is at least kMlaVarlenMinSplitTiles = 8 key tiles long, not 4: the combine's packed path costs more per split than the fixed
// one, and the split sweep of benchmarks/bench_mla_varlen.py has 8-tile splits ahead of 4-tile ones, outside both sides' ranges,
// wherever the two differ ("MLA decode: packed queries").  Every other shape is counted as
// fa2_kvcache_varlen_num_splits counts the VALU form.
constexpr int kMlaVarlenMinSplitTiles = 8;

int num_splits_mla_varlen(const SplitShape &s) {
    if (!fa2_decode_mla16_shape(s.d, s.d_v, s.dtype) || s.H_kv < 1 || s.H % s.H_kv != 0) {
        SplitShape valu = s;
        valu.d = 0;
        return num_splits_varlen(valu);
    }
    const int64_t g = s.H / s.H_kv;
    const int64_t grid = s.B * ((g * s.N_q + 63) / 64), packed = (g * s.total_q + 63) / 64 + s.B;
    return split_count(s.H_kv * (grid < packed ? grid : packed), s.S_k, kMlaSplitWaves, kMlaVarlenMinSplitTiles);
}

// fa2_kvcache_mla_sparse_num_splits: num_splits_mla with the list's topk slots in S_k's place -- the splits run over slots -- and the
// unsplit launch of the list-addressed latent form (fa2_decode_mla16_s.hip), B * N_q * H_kv * ceil(g / 64) workgroups: a workgroup
// owns the heads of ONE query position.  The same constants: one wave of the chip, four tiles per split.  Every other shape is
// counted as the VALU form's (fa2_decode_sparse_generic.hip), B * N_q * H_kv * ceil(g / 16) workgroups.
int num_splits_mla_sparse(const SplitShape &s) {
    if (s.H_kv < 1 || s.H % s.H_kv != 0) return 1;
    const int64_t g = s.H / s.H_kv, tok = s.B * s.N_q * s.H_kv;
    if (!fa2_decode_mla16_shape(s.d, s.d_v, s.dtype)) return split_count(tok * ((g + 15) / 16), s.S_k, kSplitWaves, kMinSplitTiles);
    return split_count(tok * ((g + 63) / 64), s.S_k, kMlaSplitWaves, kMlaMinSplitTiles);
}

// fa2_kvcache_mla_sparse_varlen_num_splits: num_splits_mla_sparse on total_q packed rows in B * N_q's place.  Both packed forms give a
// workgroup ONE packed row, so the unsplit count is total_q * H_kv * head tiles however the rows fall into sequences.
int num_splits_mla_sparse_varlen(const SplitShape &s) {
    SplitShape rows = s;
    rows.B = s.total_q;
    rows.N_q = 1;
    return num_splits_mla_sparse(rows);
}

// The fp32 workspace of a split call: o_part [num_splits][rows][d_v] then l_part [num_splits][rows], rows = B * H * N_q
// (total_q * H for packed queries).
int64_t workspace_bytes(int64_t rows, int64_t d_v, int64_t num_splits) {
    if (num_splits <= 1) return 0;
    if (num_splits > FA2_KVCACHE_MAX_SPLITS) num_splits = FA2_KVCACHE_MAX_SPLITS;
    if (rows > kMaxRows || d_v > 512) return INT64_MAX;  // (4 * 128 * 2^40 * 513 < 2^63)
    return 4 * num_splits * rows * (d_v + 1);
}

// The arguments of an attention call as the entry points take them.  The strides are the fixed call's: {batch, head, token, d} and
// {batch, head}; a packed entry point converts its own (packed4) and passes max_seqlen_q as N_q.
struct DecodeCall {
    const void *Q, *K, *V;
    void *O, *L;
    const int64_t *q_strides, *k_strides, *v_strides, *o_strides, *l_strides;
    const int32_t *cache_seqlens;
    int32_t B, H, H_kv, N_q, S_k, d, dtype_enum, causal, window_left, window_right, num_splits, variant;
    float scale;
    void *workspace, *hip_stream;
    int64_t workspace_bytes;
    // the optional parts, each behind its flag
    const int32_t *block_table = nullptr;  // a paged cache: S_k is ignored and max_blocks * page_size takes its place
    bool pool_only = false;                // fa2_fwd_kvcache_paged: a null block_table is refused, it is no contiguous cache
    int64_t block_table_stride = 0;
    int32_t num_blocks = 0, page_size = 0, max_blocks = 0;
    bool fp8 = false;  // an fp8 cache in kv_dtype_enum with its descales; without it the cache has dtype_enum and they are null
    int32_t kv_dtype_enum = 0;
    const float *k_descale = nullptr, *v_descale = nullptr;
    const int64_t *k_descale_strides = nullptr, *v_descale_strides = nullptr;
    bool packed = false;  // fa2_fwd_kvcache_varlen, _mla_varlen (with `mla`): Q, O are (total_q, H, d) over cu_seqlens_q, L is (H, total_q)
    const int32_t *cu_seqlens_q = nullptr;
    int32_t total_q = 0, max_seqlen_q = 0;
    // fa2_fwd_kvcache_mla_sparse (with `mla`): every (b, h_kv, position) attends over its own list of key indices; with `packed`
    // (fa2_fwd_kvcache_mla_sparse_varlen) every (packed row, h_kv), index_strides already {0, KV head, token, slot}
    bool sparse = false;
    const int32_t *indices = nullptr;
    const int64_t *index_strides = nullptr;
    int32_t topk = 0;
    bool mla = false;  // fa2_fwd_kvcache_mla, _mla_fp8 (with `fp8`), _mla_varlen (with `packed`): V is (B, H_kv, S_k, d_v), d may reach 576; without it d_v = d
    int32_t d_v = 0;
};

// The six forms of the call: fixed N_q, packed queries (query-tiled), the latent cache, packed queries over the latent cache, key
// lists over the latent cache, key lists of packed queries over the latent cache.  Each has a matrix kernel of its own beside a VALU kernel (`generic`: fa2_launch_decode_generic, the
// lists their own) and the combine, which all share; `variant` is the id that forces the matrix kernel, and AUTO, GENERIC and that id
// are the variants the form accepts: any other gets `unknown_variant`.
struct DecodeForm {
    bool (*supports)(const Fa2DecodeProblem &);
    int (*launch)(const Fa2DecodeProblem &);
    int32_t variant;
    const char *unknown_variant;
    int (*generic)(const Fa2DecodeProblem &) = fa2_launch_decode_generic;
};
const DecodeForm kForms[6] = {
    {fa2_decode_mfma16_supports, fa2_launch_decode_mfma16, FA2_KVCACHE_VARIANT_MFMA16, "kvcache: unknown variant %d (auto 0, generic 1, mfma16 2)"},
    {fa2_decode_mfma16_v_supports, fa2_launch_decode_mfma16_v, FA2_KVCACHE_VARIANT_MFMA16, "kvcache: unknown variant %d (auto 0, generic 1, mfma16 2)"},
    {fa2_decode_mla16_supports, fa2_launch_decode_mla16, FA2_KVCACHE_VARIANT_MLA16, "kvcache mla: unknown variant %d (auto 0, generic 1, mla16 3)"},
    {fa2_decode_mla16_v_supports, fa2_launch_decode_mla16_v, FA2_KVCACHE_VARIANT_MLA16, "kvcache mla: unknown variant %d (auto 0, generic 1, mla16 3)"},
    {fa2_decode_mla16_s_supports, fa2_launch_decode_mla16_s, FA2_KVCACHE_VARIANT_MLA16, "kvcache mla sparse: unknown variant %d (auto 0, generic 1, mla16 3)",
     fa2_launch_decode_sparse_generic},
    {fa2_decode_mla16_sv_supports, fa2_launch_decode_mla16_sv, FA2_KVCACHE_VARIANT_MLA16, "kvcache mla sparse: unknown variant %d (auto 0, generic 1, mla16 3)",
     fa2_launch_decode_sparse_generic_v},
};
const DecodeForm &form_of(const DecodeCall &c) {
    return kForms[c.sparse && c.packed ? 5 : c.sparse ? 4 : c.packed && c.mla ? 3 : c.mla ? 2 : c.packed ? 1 : 0];
}

// The sizes of a paged cache, for check_decode ("kvcache paged") and check_append ("kvcache append"); on FA2_OK `cap` is the capacity.
int check_paged(const char *who, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int64_t table_stride, int64_t &cap) {
    if (num_blocks < 1 || page_size < 1 || max_blocks < 1) {
        fa2_set_error("%s: num_blocks, page_size and max_blocks must be >= 1 (got num_blocks=%d, page_size=%d, max_blocks=%d)", who,
                      num_blocks, page_size, max_blocks);
        return FA2_ERR_BAD_ARG;
    }
    cap = (int64_t)max_blocks * page_size;
    if (cap > (1 << 28)) {
        fa2_set_error("%s: the capacity max_blocks * page_size must be <= 2^28 (got %lld)", who, (long long)cap);
        return FA2_ERR_BAD_ARG;
    }
    if (table_stride < 0) {
        fa2_set_error("%s: negative block_table_stride", who);
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

// The descales of an fp8 cache and their strides, for check_decode ("kvcache fp8") and check_append ("kvcache append").
int check_descales(const char *who, const float *kd, const int64_t *kds, const float *vd, const int64_t *vds) {
    if ((kd && !kds) || (vd && !vds)) {
        fa2_set_error("%s: null %s with a non-null descale", who, kd && !kds ? "k_descale_strides" : "v_descale_strides");
        return FA2_ERR_BAD_ARG;
    }
    if ((kd && (kds[0] < 0 || kds[1] < 0)) || (vd && (vds[0] < 0 || vds[1] < 0))) {
        fa2_set_error("%s: negative strides are not supported (k_descale_strides, v_descale_strides)", who);
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

// Every check of an attention call, before any launch; on FA2_OK `p` is the problem to launch, num_splits resolved.
int check_decode(const DecodeCall &c, Fa2DecodeProblem &p) {
    if (c.packed) {  // what only the packed queries bring comes first
        if (!c.q_strides || !c.o_strides) {
            fa2_set_error("kvcache varlen: null %s", !c.q_strides ? "q_strides" : "o_strides");
            return FA2_ERR_BAD_ARG;
        }
        if (!c.cu_seqlens_q) {
            fa2_set_error("kvcache varlen: null cu_seqlens_q");
            return FA2_ERR_BAD_ARG;
        }
        if (c.total_q < 1) {
            fa2_set_error("kvcache varlen: total_q must be >= 1 (got %d)", c.total_q);
            return FA2_ERR_BAD_ARG;
        }
        if (c.max_seqlen_q < 1 || c.max_seqlen_q > (1 << 28)) {
            fa2_set_error("kvcache varlen: max_seqlen_q must be in [1, 2^28] (got %d)", c.max_seqlen_q);
            return FA2_ERR_BAD_ARG;
        }
        if (c.H >= 1 && (int64_t)c.total_q * c.H > kMaxRows) {
            fa2_set_error("kvcache varlen: total_q * H must be <= 2^40 (got %lld)", (long long)c.total_q * c.H);
            return FA2_ERR_BAD_ARG;
        }
        if (c.l_strides[1] < 0) {
            fa2_set_error("kvcache: negative strides are not supported (l_head_stride)");
            return FA2_ERR_BAD_ARG;
        }
    }
    if (c.sparse) {  // what only the key lists bring comes first
        if (!c.indices || !c.index_strides) {
            fa2_set_error("kvcache mla sparse: null %s", !c.indices ? "indices" : "index_strides");
            return FA2_ERR_BAD_ARG;
        }
        for (int k = 0; k < 4; ++k)
            if (c.index_strides[k] < 0) {
                fa2_set_error("kvcache mla sparse: negative strides are not supported (index_strides)");
                return FA2_ERR_BAD_ARG;
            }
        if (c.topk < 1 || c.topk > (1 << 28)) {
            fa2_set_error("kvcache mla sparse: topk must be in [1, 2^28] (got %d)", c.topk);
            return FA2_ERR_BAD_ARG;
        }
        if (c.fp8 && (!c.k_descale || !c.v_descale)) {  // (the other calls read a null descale as 1: a quantised cache has one)
            fa2_set_error("kvcache mla sparse: null %s with an fp8 cache (kv_dtype_enum %d)", !c.k_descale ? "k_descale" : "v_descale",
                          c.kv_dtype_enum);
            return FA2_ERR_BAD_ARG;
        }
    }
    if (!c.fp8 && (c.k_descale || c.v_descale)) {  // (a fused step has refused them in check_append)
        fa2_set_error(c.packed ? "kvcache varlen: k_descale / v_descale go with an fp8 cache (kv_dtype_enum %d == dtype_enum)"
                               : "kvcache paged: k_descale / v_descale go with an fp8 pool (kv_dtype_enum %d == dtype_enum)",
                      c.kv_dtype_enum);
        return FA2_ERR_BAD_ARG;
    }
    const void *ptrs[10] = {c.Q, c.K, c.V, c.O, c.L, c.q_strides, c.k_strides, c.v_strides, c.o_strides, c.l_strides};
    const char *names[10] = {"Q", "K", "V", "O", "L", "q_strides", "k_strides", "v_strides", "o_strides", "l_strides"};
    for (int t = 0; t < 10; ++t)
        if (!ptrs[t]) {
            fa2_set_error("kvcache: null %s", names[t]);
            return FA2_ERR_BAD_ARG;
        }
    int64_t cap = c.S_k;
    const bool paged = c.pool_only || c.block_table;
    if (paged) {
        if (!c.block_table) {
            fa2_set_error("kvcache paged: null block_table");
            return FA2_ERR_BAD_ARG;
        }
        const int rc = check_paged("kvcache paged", c.num_blocks, c.page_size, c.max_blocks, c.block_table_stride, cap);
        if (rc != FA2_OK) return rc;
    }
    const int32_t S_k = (int32_t)cap;
    if (c.B < 1 || c.B > 65535) {
        fa2_set_error("kvcache: B must be in [1, 65535] (got %d)", c.B);
        return FA2_ERR_BAD_ARG;
    }
    if (c.H < 1 || c.H > 65535) {
        fa2_set_error("kvcache: H must be in [1, 65535] (got %d)", c.H);
        return FA2_ERR_BAD_ARG;
    }
    const int gqa = fa2_check_gqa(c.H, c.H_kv);
    if (gqa != FA2_OK) return gqa;
    if (!c.packed && (c.N_q < 1 || c.N_q > (1 << 28))) {
        fa2_set_error("kvcache: N_q must be in [1, 2^28] (got %d)", c.N_q);
        return FA2_ERR_BAD_ARG;
    }
    if (S_k < 1 || S_k > (1 << 28)) {
        fa2_set_error("kvcache: S_k must be in [1, 2^28] (got %d)", S_k);
        return FA2_ERR_BAD_ARG;
    }
    if (!c.packed && (int64_t)c.B * c.H * c.N_q > kMaxRows) {
        fa2_set_error("kvcache: B * H * N_q must be <= 2^40 (got %lld)", (long long)c.B * c.H * c.N_q);
        return FA2_ERR_BAD_ARG;
    }
    if (c.window_left < -1 || c.window_right < -1) {
        fa2_set_error("window sides must be >= -1 (-1 = unbounded), got window=(%d, %d)", c.window_left, c.window_right);
        return FA2_ERR_BAD_ARG;
    }
    for (int k = 0; k < 4; ++k)
        if (c.q_strides[k] < 0 || c.k_strides[k] < 0 || c.v_strides[k] < 0 || c.o_strides[k] < 0) {
            fa2_set_error("kvcache: negative strides are not supported");
            return FA2_ERR_BAD_ARG;
        }
    if (c.l_strides[0] < 0 || c.l_strides[1] < 0) {
        fa2_set_error("kvcache: negative strides are not supported (l_strides)");
        return FA2_ERR_BAD_ARG;
    }
    if (!(c.scale == c.scale)) {
        fa2_set_error("kvcache: scale is NaN");
        return FA2_ERR_BAD_ARG;
    }
    if (c.num_splits < 0 || c.num_splits > FA2_KVCACHE_MAX_SPLITS) {
        fa2_set_error("kvcache: num_splits must be in [0, %d] (0 = auto), got %d", FA2_KVCACHE_MAX_SPLITS, c.num_splits);
        return FA2_ERR_BAD_ARG;
    }
    if (c.fp8) {
        const int rc = check_descales("kvcache fp8", c.k_descale, c.k_descale_strides, c.v_descale, c.v_descale_strides);
        if (rc != FA2_OK) return rc;
        if (c.kv_dtype_enum != FA2_DTYPE_F8E4M3 && c.kv_dtype_enum != FA2_DTYPE_F8E5M2) {
            fa2_set_error("kvcache fp8: kv_dtype_enum %d must be FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2", c.kv_dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.dtype_enum != FA2_DTYPE_F16 && c.dtype_enum != FA2_DTYPE_BF16) {
            fa2_set_error("kvcache fp8: dtype_enum %d (Q, O, L) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16", c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
    } else if (c.dtype_enum == FA2_DTYPE_F8E5M2 || c.dtype_enum == FA2_DTYPE_F8E4M3) {
        fa2_set_error("kvcache: fp8 is not supported (e4m3fn cannot hold L = +inf)");
        return FA2_ERR_UNSUPPORTED;
    }
    if (fa2_dtype_size(c.dtype_enum) == 0) {
        fa2_set_error("unknown dtype enum %d", c.dtype_enum);
        return FA2_ERR_UNSUPPORTED;
    }
    const int32_t d_v = c.mla ? c.d_v : c.d;
    if (c.d < 1 || c.d > (c.mla ? 576 : 512)) {
        fa2_set_error(c.mla ? "kvcache mla: d=%d must be in [1, 576]" : "d=%d must be in [1, 512]", c.d);
        return FA2_ERR_UNSUPPORTED;
    }
    if (d_v < 1 || d_v > 512) {  // (the latent cache alone: elsewhere d_v is d)
        fa2_set_error("kvcache mla: d_v=%d must be in [1, 512]", d_v);
        return FA2_ERR_UNSUPPORTED;
    }
    const DecodeForm &form = form_of(c);
    if (c.variant != FA2_KVCACHE_VARIANT_AUTO && c.variant != FA2_KVCACHE_VARIANT_GENERIC && c.variant != form.variant) {
        fa2_set_error(form.unknown_variant, c.variant);
        return FA2_ERR_UNSUPPORTED;
    }

    p.Q = c.Q; p.K = c.K; p.V = c.V; p.O = c.O; p.L = c.L;
    for (int k = 0; k < 4; ++k) { p.qs[k] = c.q_strides[k]; p.ks[k] = c.k_strides[k]; p.vs[k] = c.v_strides[k]; p.os[k] = c.o_strides[k]; }
    p.ls[0] = c.l_strides[0]; p.ls[1] = c.l_strides[1];
    p.seqlens = c.cache_seqlens;
    p.B = c.B; p.H = c.H; p.H_kv = c.H_kv; p.N_q = c.N_q; p.S_k = S_k; p.d = c.d; p.d_v = d_v;
    p.kv_dtype = c.fp8 ? c.kv_dtype_enum : c.dtype_enum;
    p.kd = c.fp8 ? c.k_descale : nullptr; p.vd = c.fp8 ? c.v_descale : nullptr;
    for (int k = 0; k < 2; ++k) { p.kds[k] = p.kd ? c.k_descale_strides[k] : 0; p.vds[k] = p.vd ? c.v_descale_strides[k] : 0; }
    p.table = c.block_table;
    p.table_stride = paged ? c.block_table_stride : 0; p.page_size = paged ? c.page_size : 0; p.num_blocks = paged ? c.num_blocks : 0;
    p.dtype = c.dtype_enum; p.causal = c.causal != 0; p.wl = c.window_left; p.wr = c.window_right; p.scale = c.scale;
    p.cu_q = c.packed ? c.cu_seqlens_q : nullptr;
    p.total_q = c.packed ? c.total_q : 0; p.max_q = c.packed ? c.max_seqlen_q : 0;
    p.indices = c.sparse ? c.indices : nullptr; p.topk = c.sparse ? c.topk : 0;
    for (int k = 0; k < 4; ++k) p.is[k] = c.sparse ? c.index_strides[k] : 0;
    const SplitShape shape = {c.B, c.H, c.H_kv, c.N_q, c.total_q, c.sparse ? c.topk : S_k, c.d, d_v, c.dtype_enum};  // (the lists: splits over slots)
    p.num_splits = c.num_splits != 0 ? c.num_splits : c.sparse && c.packed ? num_splits_mla_sparse_varlen(shape) : c.sparse ? num_splits_mla_sparse(shape) : c.packed && c.mla ? num_splits_mla_varlen(shape) : c.mla ? num_splits_mla(shape) : c.packed ? num_splits_varlen(shape) : num_splits_auto(shape);
    p.stream = (hipStream_t)c.hip_stream;
    p.o_part = nullptr; p.l_part = nullptr;
    if (p.num_splits > 1) {
        const int64_t rows = c.packed ? (int64_t)c.total_q * c.H : (int64_t)c.B * c.H * c.N_q;
        const int64_t need = workspace_bytes(rows, d_v, p.num_splits);
        if (!c.workspace || c.workspace_bytes < need) {
            fa2_set_error("kvcache: workspace of %lld bytes needed for num_splits=%d (%s), got %s%lld", (long long)need, p.num_splits,
                          c.packed ? "fa2_kvcache_varlen_workspace_bytes" : "fa2_kvcache_workspace_bytes", c.workspace ? "" : "null, ",
                          (long long)c.workspace_bytes);
            return FA2_ERR_BAD_ARG;
        }
        p.o_part = (float *)c.workspace;
        p.l_part = p.o_part + (int64_t)p.num_splits * rows * d_v;
    }
    return FA2_OK;
}

// The launches of a checked call, on its stream: the append of a fused step (`append` non-null) first, then the split kernel of the
// form the variant names -- AUTO: the call's matrix form where it runs, else the VALU form -- then the combine.  A forced matrix
// form that cannot run fails (in its launcher, which names the rule) before the cache is touched.
int run_decode(const DecodeCall &c, const Fa2DecodeProblem &p, const Fa2AppendProblem *append) {
    const DecodeForm &form = form_of(c);
    const bool matrix = c.variant == FA2_KVCACHE_VARIANT_AUTO ? form.supports(p) : c.variant == form.variant;
    if (append) {
        if (matrix && !form.supports(p)) return form.launch(p);
        const int rc = fa2_launch_decode_append(*append);
        if (rc != FA2_OK) return rc;
    }
    const int rc = matrix ? form.launch(p) : form.generic(p);
    if (rc != FA2_OK || p.num_splits == 1) return rc;
    return fa2_launch_decode_combine(p);
}

// Steps 2 and 3 of an attention call; `append` is the checked cache update of a fused step, or null.
int decode(const DecodeCall &c, const Fa2AppendProblem *append) {
    Fa2DecodeProblem p;
    const int rc = check_decode(c, p);
    return rc != FA2_OK ? rc : run_decode(c, p, append);
}

// The arguments of fa2_kvcache_append as the entry points take them.
struct AppendCall {
    void *K, *V;
    const int64_t *k_strides, *v_strides;
    const int32_t *block_table;
    int64_t block_table_stride;
    const void *k_new, *v_new;
    const int64_t *k_new_strides, *v_new_strides;
    const int32_t *cache_seqlens;
    int32_t *seqlens_out;
    const float *k_descale, *v_descale;
    const int64_t *k_descale_strides, *v_descale_strides;
    const void *rotary_cos, *rotary_sin;
    int64_t cos_stride, sin_stride;
    int32_t S_rot, rotary_dim, rotary_interleaved;
    const void *Q;
    void *q_rot;
    const int64_t *q_strides;
    int32_t H, N_q, q_pos_per_row;
    int32_t B, H_kv, N_new, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum;
    void *hip_stream;
    // fa2_kvcache_append_varlen: packed tokens over cu_seqlens_new, the strides of k_new, v_new and Q already in the fixed call's
    // order {0, head, token, d} (packed4); N_new and N_q are then not looked at
    bool packed = false;
    const int32_t *cu_seqlens_new = nullptr;
    int32_t total_new = 0, max_seqlen_new = 0;
    // fa2_kvcache_mla_append, fa2_kvcache_mla_append_varlen: K is the one tensor of the latent cache (KV) and V, v_strides are null;
    // k_new / k_new_strides are c_new's, v_new / v_new_strides pe_new's, k_descale / k_descale_strides the row's kv_descale, and
    // v_descale is null.  d may reach 576 and the rotary range is [d_v, d_v + rotary_dim).
    bool mla = false;
    int32_t d_v = 0;
};

// The {token, head, d} strides of a packed tensor in the fixed call's order {batch, head, token, d}, the batch stride 0; null stays null.
const int64_t *packed4(const int64_t *s3, int64_t (&s4)[4]) {
    if (!s3) return nullptr;
    s4[0] = 0; s4[1] = s3[1]; s4[2] = s3[0]; s4[3] = s3[2];
    return s4;
}

// Every check of fa2_kvcache_append and fa2_kvcache_append_varlen, before any launch; on FA2_OK `p` is the problem to launch.
int check_append(const AppendCall &c, Fa2AppendProblem &p) {
    const void *ptrs[10] = {c.K, c.V, c.k_strides, c.v_strides, c.k_new, c.v_new, c.k_new_strides, c.v_new_strides, c.cache_seqlens,
                            c.seqlens_out};
    const char *names[10] = {"K", "V", "k_strides", "v_strides", "k_new", "v_new", "k_new_strides", "v_new_strides", "cache_seqlens",
                             "seqlens_out"};
    const char *mla_names[10] = {"KV", nullptr, "kv_strides", nullptr, "c_new", "pe_new", "c_new_strides", "pe_new_strides",
                                 "cache_seqlens", "seqlens_out"};  // (null: the latent cache has no tensor of V's)
    for (int t = 0; t < 10; ++t)
        if (!ptrs[t] && !(c.mla && !mla_names[t])) {
            fa2_set_error("kvcache append: null %s", c.mla ? mla_names[t] : names[t]);
            return FA2_ERR_BAD_ARG;
        }
    if (c.seqlens_out == c.cache_seqlens) {
        fa2_set_error("kvcache append: seqlens_out must not be cache_seqlens (the call does not modify its lengths)");
        return FA2_ERR_BAD_ARG;
    }
    int64_t cap = c.S_k;
    if (c.block_table) {
        const int rc = check_paged("kvcache append", c.num_blocks, c.page_size, c.max_blocks, c.block_table_stride, cap);
        if (rc != FA2_OK) return rc;
    } else if (cap < 1 || cap > (1 << 28)) {
        fa2_set_error("kvcache append: S_k must be in [1, 2^28] (got %d)", c.S_k);
        return FA2_ERR_BAD_ARG;
    }
    if (c.B < 1 || c.B > 65535) {
        fa2_set_error("kvcache append: B must be in [1, 65535] (got %d)", c.B);
        return FA2_ERR_BAD_ARG;
    }
    if (c.H_kv < 1 || c.H_kv > 65535) {
        fa2_set_error("kvcache append: H_kv must be in [1, 65535] (got %d)", c.H_kv);
        return FA2_ERR_BAD_ARG;
    }
    if (c.packed) {
        if (!c.cu_seqlens_new) {
            fa2_set_error("kvcache append varlen: null cu_seqlens_new");
            return FA2_ERR_BAD_ARG;
        }
        if (c.total_new < 1 || c.total_new > (1 << 28)) {
            fa2_set_error("kvcache append varlen: total_new must be in [1, 2^28] (got %d)", c.total_new);
            return FA2_ERR_BAD_ARG;
        }
        if (c.max_seqlen_new < 1 || c.max_seqlen_new > (1 << 28)) {
            fa2_set_error("kvcache append varlen: max_seqlen_new must be in [1, 2^28] (got %d)", c.max_seqlen_new);
            return FA2_ERR_BAD_ARG;
        }
    } else if (c.N_new < 1 || c.N_new > (1 << 28)) {
        fa2_set_error("kvcache append: N_new must be in [1, 2^28] (got %d)", c.N_new);
        return FA2_ERR_BAD_ARG;
    }
    if (c.Q) {
        if (!c.q_strides) {
            fa2_set_error("kvcache append: null q_strides with a non-null Q");
            return FA2_ERR_BAD_ARG;
        }
        if (c.H < 1 || c.H > 65535) {
            fa2_set_error("kvcache append: H must be in [1, 65535] (got %d)", c.H);
            return FA2_ERR_BAD_ARG;
        }
        const int rc = fa2_check_gqa(c.H, c.H_kv);
        if (rc != FA2_OK) return rc;
        if (!c.packed && (c.N_q < 1 || c.N_q > (1 << 28))) {
            fa2_set_error("kvcache append: N_q must be in [1, 2^28] (got %d)", c.N_q);
            return FA2_ERR_BAD_ARG;
        }
    }
    if (c.packed) {  // the rows one packed launch walks, held to the bound of B * H * N_q: a row's byte offset stays below 2^52
        const int64_t slabs = c.Q && c.H > 2 * c.H_kv ? c.H : 2 * c.H_kv;
        if (c.total_new * slabs > kMaxRows) {
            fa2_set_error("kvcache append varlen: total_new * max(H, 2 * H_kv) must be <= 2^40 (got %lld)", (long long)(c.total_new * slabs));
            return FA2_ERR_BAD_ARG;
        }
    }
    for (int k = 0; k < 4; ++k)
        if (c.k_strides[k] < 0 || (!c.mla && c.v_strides[k] < 0) || c.k_new_strides[k] < 0 || c.v_new_strides[k] < 0 ||
            (c.Q && c.q_strides[k] < 0)) {
            fa2_set_error(c.mla ? "kvcache append: negative strides are not supported (kv_strides, c_new_strides, pe_new_strides, q_strides)"
                                : "kvcache append: negative strides are not supported (k_strides, v_strides, k_new_strides, v_new_strides, "
                                  "q_strides)");
            return FA2_ERR_BAD_ARG;
        }
    const bool wide = c.kv_dtype_enum == c.dtype_enum;  // the cache has the inputs' dtype
    if (wide) {
        if (c.k_descale || c.v_descale) {
            fa2_set_error(c.mla ? "kvcache append: kv_descale goes with an fp8 cache (kv_dtype_enum %d == dtype_enum)"
                                : "kvcache append: k_descale / v_descale go with an fp8 cache (kv_dtype_enum %d == dtype_enum)",
                          c.kv_dtype_enum);
            return FA2_ERR_BAD_ARG;
        }
        if (c.dtype_enum == FA2_DTYPE_F8E5M2 || c.dtype_enum == FA2_DTYPE_F8E4M3) {
            fa2_set_error("kvcache append: dtype_enum %d: fp8 inputs are not supported (an fp8 cache takes f16 / bf16 inputs)", c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
    } else {
        if (c.mla && c.k_descale && (!c.k_descale_strides || c.k_descale_strides[0] < 0 || c.k_descale_strides[1] < 0)) {
            fa2_set_error(c.k_descale_strides ? "kvcache append: negative strides are not supported (kv_descale_strides)"
                                              : "kvcache append: null kv_descale_strides with a non-null kv_descale");
            return FA2_ERR_BAD_ARG;
        }
        const int rc = check_descales("kvcache append", c.k_descale, c.k_descale_strides, c.v_descale, c.v_descale_strides);
        if (rc != FA2_OK) return rc;
        if (c.kv_dtype_enum != FA2_DTYPE_F8E4M3 && c.kv_dtype_enum != FA2_DTYPE_F8E5M2) {
            fa2_set_error("kvcache append: kv_dtype_enum %d must be dtype_enum, FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2", c.kv_dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.dtype_enum != FA2_DTYPE_F16 && c.dtype_enum != FA2_DTYPE_BF16) {
            fa2_set_error(c.mla ? "kvcache append: dtype_enum %d (c_new, pe_new, Q) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16 under an fp8 cache"
                                : "kvcache append: dtype_enum %d (k_new, v_new, Q) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16 under an fp8 cache",
                          c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
    }
    if (fa2_dtype_size(c.dtype_enum) == 0) {
        fa2_set_error("unknown dtype enum %d", c.dtype_enum);
        return FA2_ERR_UNSUPPORTED;
    }
    if (c.mla) {
        if (c.d < 2 || c.d > 576) {
            fa2_set_error("kvcache mla append: d=%d must be in [2, 576]", c.d);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.d_v < 1 || c.d_v > c.d - 1) {
            fa2_set_error("kvcache mla append: d_v=%d must be in [1, d - 1 = %d]", c.d_v, c.d - 1);
            return FA2_ERR_UNSUPPORTED;
        }
    } else if (c.d < 1 || c.d > 512) {
        fa2_set_error("d=%d must be in [1, 512]", c.d);
        return FA2_ERR_UNSUPPORTED;
    }
    const int32_t rotary_max = c.mla ? c.d - c.d_v : c.d;  // the columns the rotary range may take
    const bool rotary = c.rotary_cos || c.rotary_sin;
    if (rotary) {
        if (!c.rotary_cos || !c.rotary_sin) {
            fa2_set_error("kvcache append: rotary_cos and rotary_sin go together (null %s)", c.rotary_cos ? "rotary_sin" : "rotary_cos");
            return FA2_ERR_BAD_ARG;
        }
        if (c.rotary_dim < 2 || c.rotary_dim > rotary_max || (c.rotary_dim & 1)) {
            fa2_set_error(c.mla ? "kvcache append: rotary_dim must be even and in [2, d - d_v = %d] (got %d)"
                                : "kvcache append: rotary_dim must be even and in [2, d = %d] (got %d)", rotary_max, c.rotary_dim);
            return FA2_ERR_BAD_ARG;
        }
        if (c.S_rot < 1) {
            fa2_set_error("kvcache append: S_rot must be >= 1 (got %d)", c.S_rot);
            return FA2_ERR_BAD_ARG;
        }
        if (c.cos_stride < 0 || c.sin_stride < 0) {
            fa2_set_error("kvcache append: negative strides are not supported (rotary_cos_stride, rotary_sin_stride)");
            return FA2_ERR_BAD_ARG;
        }
        if (c.Q && !c.q_rot) {
            fa2_set_error("kvcache append: null q_rot with rotary tables and a non-null Q");
            return FA2_ERR_BAD_ARG;
        }
    }
    p.K = c.K; p.V = c.mla ? nullptr : c.V;
    for (int k = 0; k < 4; ++k) {
        p.ks[k] = c.k_strides[k]; p.vs[k] = c.mla ? 0 : c.v_strides[k]; p.kns[k] = c.k_new_strides[k]; p.vns[k] = c.v_new_strides[k];
        p.pns[k] = c.v_new_strides[k];
        p.qs[k] = c.Q ? c.q_strides[k] : 0;
    }
    p.pe_new = c.mla ? c.v_new : nullptr; p.d_v = c.mla ? c.d_v : 0;
    p.table = c.block_table;
    p.table_stride = c.block_table ? c.block_table_stride : 0;
    p.page_size = c.block_table ? c.page_size : 0; p.num_blocks = c.block_table ? c.num_blocks : 0;
    p.capacity = (int32_t)cap;
    p.k_new = c.k_new; p.v_new = c.v_new;
    p.seqlens = c.cache_seqlens; p.seqlens_out = c.seqlens_out;
    p.kd = wide ? nullptr : c.k_descale; p.vd = wide ? nullptr : c.v_descale;
    for (int k = 0; k < 2; ++k) { p.kds[k] = p.kd ? c.k_descale_strides[k] : 0; p.vds[k] = p.vd ? c.v_descale_strides[k] : 0; }
    p.cos = c.rotary_cos; p.sin = c.rotary_sin;
    p.cos_stride = rotary ? c.cos_stride : 0; p.sin_stride = rotary ? c.sin_stride : 0;
    p.S_rot = rotary ? c.S_rot : 1; p.rotary_dim = rotary ? c.rotary_dim : 0; p.interleaved = c.rotary_interleaved != 0;
    p.Q = rotary ? c.Q : nullptr;  // without tables there is nothing to do to Q
    p.q_rot = rotary ? c.q_rot : nullptr;
    p.H = c.Q ? c.H : 0; p.N_q = c.Q ? c.N_q : 0; p.q_pos_per_row = c.q_pos_per_row != 0;
    p.B = c.B; p.H_kv = c.H_kv; p.N_new = c.N_new; p.d = c.d;
    p.dtype = c.dtype_enum; p.kv_dtype = c.kv_dtype_enum;
    p.stream = (hipStream_t)c.hip_stream;
    p.cu_new = c.packed ? c.cu_seqlens_new : nullptr;
    p.total_new = c.packed ? c.total_new : 0; p.max_new = c.packed ? c.max_seqlen_new : 0;
    return FA2_OK;
}

}  // namespace

extern "C" {

int fa2_fwd_kvcache(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                    const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                    const int32_t *cache_seqlens, int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d,
                    int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                    void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return fa2_fwd_kvcache_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, cache_seqlens, B, H, H_kv, N_q,
                                   S_k, d, dtype_enum, causal, scale, window_left, window_right, num_splits, workspace, workspace_bytes,
                                   hip_stream, FA2_KVCACHE_VARIANT_AUTO);
}

int fa2_fwd_kvcache_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                            const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                            const int64_t l_strides[2], const int32_t *cache_seqlens, int32_t B, int32_t H, int32_t H_kv,
                            int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                            int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes,
                            void *hip_stream, int32_t variant) {
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides; c.l_strides = l_strides;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return decode(c, nullptr);
}

int fa2_fwd_kvcache_fp8(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                        const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                        const int32_t *cache_seqlens, const float *k_descale, const float *v_descale,
                        const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                        int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale,
                        int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes,
                        int32_t variant, void *hip_stream) {
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides; c.l_strides = l_strides;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.fp8 = true; c.kv_dtype_enum = kv_dtype_enum;  // (whatever kv_dtype_enum holds: one that is no fp8 format is refused)
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    return decode(c, nullptr);
}

int fa2_fwd_kvcache_paged(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                          const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                          const int64_t l_strides[2], const int32_t *cache_seqlens, const int32_t *block_table,
                          int64_t block_table_stride, const float *k_descale, const float *v_descale,
                          const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                          int32_t N_q, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t dtype_enum,
                          int32_t kv_dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                          int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides; c.l_strides = l_strides;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = 0; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.pool_only = true; c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;  // (a pool in Q's dtype: no descales)
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    return decode(c, nullptr);
}

int fa2_fwd_kvcache_mla(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                        const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                        const int32_t *cache_seqlens, const int32_t *block_table, int64_t block_table_stride, int32_t B, int32_t H,
                        int32_t H_kv, int32_t N_q, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                        int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                        void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides; c.l_strides = l_strides;
    // block_table null: the contiguous cache, a pool of one page per sequence: page_size carries S_k (num_blocks, max_blocks are not read)
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = block_table ? 0 : page_size; c.d = d; c.dtype_enum = dtype_enum;
    c.causal = causal; c.scale = scale; c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    return decode(c, nullptr);
}

int fa2_fwd_kvcache_mla_fp8(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                            const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                            const int64_t l_strides[2], const int32_t *cache_seqlens, const int32_t *block_table,
                            int64_t block_table_stride, const float *k_descale, const float *v_descale,
                            const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                            int32_t N_q, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                            int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale, int32_t window_left,
                            int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant,
                            void *hip_stream) {
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides; c.l_strides = l_strides;
    // (block_table null: the contiguous cache, page_size carries S_k, as in fa2_fwd_kvcache_mla)
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = block_table ? 0 : page_size; c.d = d; c.dtype_enum = dtype_enum;
    c.causal = causal; c.scale = scale; c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;  // (a cache in Q's dtype: no descales, fa2_fwd_kvcache_mla's launch)
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    return decode(c, nullptr);
}

int32_t fa2_kvcache_mla_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t d_v,
                                   int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || N_q < 1 || S_k < 1) return 1;
    return num_splits_mla({B, H, H_kv, N_q, 0, S_k, d, d_v, dtype_enum});
}

int fa2_fwd_kvcache_mla_sparse(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                               const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                               const int64_t l_strides[2], const int32_t *cache_seqlens, const int32_t *indices,
                               const int64_t index_strides[4], int32_t topk, const int32_t *block_table, int64_t block_table_stride,
                               const float *k_descale, const float *v_descale, const int64_t k_descale_strides[2],
                               const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t num_blocks,
                               int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum,
                               float scale, int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant,
                               void *hip_stream) {
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides; c.l_strides = l_strides;
    // (block_table null: the contiguous cache, page_size carries S_k, as in fa2_fwd_kvcache_mla); the list is the mask: no band
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = block_table ? 0 : page_size; c.d = d; c.dtype_enum = dtype_enum;
    c.causal = 0; c.scale = scale; c.window_left = -1; c.window_right = -1; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    c.sparse = true; c.indices = indices; c.index_strides = index_strides; c.topk = topk;
    return decode(c, nullptr);
}

int32_t fa2_kvcache_mla_sparse_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t topk, int32_t d, int32_t d_v,
                                          int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || N_q < 1 || topk < 1) return 1;
    return num_splits_mla_sparse({B, H, H_kv, N_q, 0, topk, d, d_v, dtype_enum});
}

int fa2_fwd_kvcache_mla_sparse_varlen(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                                      const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[3],
                                      int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                                      const int32_t *indices, const int64_t index_strides[3], int32_t topk, const int32_t *block_table,
                                      int64_t block_table_stride, const float *k_descale, const float *v_descale,
                                      const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H,
                                      int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t num_blocks, int32_t page_size,
                                      int32_t max_blocks, int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum, float scale,
                                      int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    // the packed tensors in the fixed call's terms, as in fa2_fwd_kvcache_mla_varlen; the lists {token, KV head, slot} alike: no batch
    // stride, the token axis where the query position is
    int64_t qs[4], os[4], is[4];
    const int64_t ls[2] = {0, l_head_stride};
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = packed4(q_strides, qs); c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = packed4(o_strides, os);
    c.l_strides = ls;
    // (block_table null: the contiguous cache, page_size carries S_k, as in fa2_fwd_kvcache_mla_sparse); the list is the mask: no band
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = max_seqlen_q; c.S_k = block_table ? 0 : page_size; c.d = d; c.dtype_enum = dtype_enum;
    c.causal = 0; c.scale = scale; c.window_left = -1; c.window_right = -1; c.num_splits = num_splits;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    c.packed = true; c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    c.sparse = true; c.indices = indices; c.topk = topk;
    c.index_strides = index_strides ? is : nullptr;
    if (index_strides) { is[0] = 0; is[1] = index_strides[1]; is[2] = index_strides[0]; is[3] = index_strides[2]; }
    return decode(c, nullptr);
}

int32_t fa2_kvcache_mla_sparse_varlen_num_splits(int32_t total_q, int32_t H, int32_t H_kv, int32_t topk, int32_t d, int32_t d_v,
                                                 int32_t dtype_enum) {
    if (total_q < 1 || H < 1 || H_kv < 1 || topk < 1) return 1;
    return num_splits_mla_sparse_varlen({1, H, H_kv, 1, total_q, topk, d, d_v, dtype_enum});
}

int fa2_fwd_kvcache_varlen(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                           const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[3], int64_t l_head_stride,
                           const int32_t *cu_seqlens_q, const int32_t *cache_seqlens, const int32_t *block_table,
                           int64_t block_table_stride, const float *k_descale, const float *v_descale,
                           const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                           int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size, int32_t max_blocks,
                           int32_t d, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale, int32_t window_left,
                           int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant,
                           void *hip_stream) {
    // the packed tensors in the fixed call's terms: no batch stride, the token axis where the query position is
    int64_t qs[4], os[4];
    const int64_t ls[2] = {0, l_head_stride};
    DecodeCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = packed4(q_strides, qs); c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = packed4(o_strides, os);
    c.l_strides = ls;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = max_seqlen_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    c.packed = true; c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    return decode(c, nullptr);
}

int64_t fa2_kvcache_varlen_workspace_bytes(int32_t total_q, int32_t H, int32_t d, int32_t num_splits) {
    if (total_q < 1 || H < 1 || d < 1 || H > 65535) return 0;
    return workspace_bytes((int64_t)total_q * H, d, num_splits);
}

int32_t fa2_kvcache_varlen_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t d,
                                      int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || total_q < 1 || max_seqlen_q < 1 || S_k < 1) return 1;
    return num_splits_varlen({B, H, H_kv, max_seqlen_q, total_q, S_k, d, d, dtype_enum});
}

int fa2_fwd_kvcache_mla_varlen(const void *Q, const void *KV, void *O, void *L, const int64_t q_strides[3], const int64_t kv_strides[4],
                               const int64_t o_strides[3], int64_t l_head_stride, const int32_t *cu_seqlens_q,
                               const int32_t *cache_seqlens, const int32_t *block_table, int64_t block_table_stride,
                               const float *kv_descale, const int64_t kv_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                               int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size,
                               int32_t max_blocks, int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal,
                               float scale, int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace,
                               int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    // the packed tensors in the fixed call's terms, as in fa2_fwd_kvcache_varlen; V is the first d_v columns of the row K scores, the
    // one descale K's and V's, as in fa2_fwd_kvcache_mla_append
    int64_t qs[4], os[4];
    const int64_t ls[2] = {0, l_head_stride};
    DecodeCall c;
    c.Q = Q; c.K = KV; c.V = KV; c.O = O; c.L = L; c.cache_seqlens = cache_seqlens; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = packed4(q_strides, qs); c.k_strides = kv_strides; c.v_strides = kv_strides; c.o_strides = packed4(o_strides, os);
    c.l_strides = ls;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = max_seqlen_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = kv_descale; c.v_descale = kv_descale; c.k_descale_strides = kv_descale_strides; c.v_descale_strides = kv_descale_strides;
    c.packed = true; c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    return decode(c, nullptr);
}

int32_t fa2_kvcache_mla_varlen_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                                          int32_t d, int32_t d_v, int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || total_q < 1 || max_seqlen_q < 1 || S_k < 1) return 1;
    return num_splits_mla_varlen({B, H, H_kv, max_seqlen_q, total_q, S_k, d, d_v, dtype_enum});
}

int64_t fa2_kvcache_workspace_bytes(int32_t B, int32_t H, int32_t N_q, int32_t d, int32_t num_splits) {
    if (B < 1 || H < 1 || N_q < 1 || d < 1 || B > 65535 || H > 65535 || N_q > (1 << 28)) return 0;
    return workspace_bytes((int64_t)B * H * N_q, d, num_splits);
}

int32_t fa2_kvcache_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || N_q < 1 || S_k < 1) return 1;
    return num_splits_auto({B, H, H_kv, N_q, 0, S_k, d, d, dtype_enum});
}

int fa2_kvcache_append(void *K, void *V, const int64_t k_strides[4], const int64_t v_strides[4], const int32_t *block_table,
                       int64_t block_table_stride, const void *k_new, const void *v_new, const int64_t k_new_strides[4],
                       const int64_t v_new_strides[4], const int32_t *cache_seqlens, int32_t *seqlens_out, const float *k_descale,
                       const float *v_descale, const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                       const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                       int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, const void *Q, void *q_rot,
                       const int64_t q_strides[4], int32_t H, int32_t N_q, int32_t q_pos_per_row, int32_t B, int32_t H_kv,
                       int32_t N_new, int32_t S_k, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                       int32_t dtype_enum, int32_t kv_dtype_enum, void *hip_stream) {
    const AppendCall c = {K, V, k_strides, v_strides, block_table, block_table_stride, k_new, v_new, k_new_strides, v_new_strides,
                          cache_seqlens, seqlens_out, k_descale, v_descale, k_descale_strides, v_descale_strides, rotary_cos, rotary_sin,
                          rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot, q_strides, H, N_q,
                          q_pos_per_row, B, H_kv, N_new, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum, hip_stream};
    Fa2AppendProblem p;
    const int rc = check_append(c, p);
    return rc != FA2_OK ? rc : fa2_launch_decode_append(p);
}

int fa2_fwd_kvcache_append(const void *Q, void *K, void *V, void *O, void *L, const int64_t q_strides[4], const int64_t k_strides[4],
                           const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                           const int32_t *cache_seqlens, int32_t *seqlens_out, const int32_t *block_table, int64_t block_table_stride,
                           const float *k_descale, const float *v_descale, const int64_t k_descale_strides[2],
                           const int64_t v_descale_strides[2], const void *k_new, const void *v_new, const int64_t k_new_strides[4],
                           const int64_t v_new_strides[4], const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride,
                           int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, void *q_rot,
                           int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t N_new, int32_t S_k, int32_t num_blocks,
                           int32_t page_size, int32_t max_blocks, int32_t d, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal,
                           float scale, int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace,
                           int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    const int32_t per_row = causal || window_left >= 0 || window_right >= 0;  // flash-attn's rule for Q's rotary positions
    const AppendCall a = {K, V, k_strides, v_strides, block_table, block_table_stride, k_new, v_new, k_new_strides, v_new_strides,
                          cache_seqlens, seqlens_out, k_descale, v_descale, k_descale_strides, v_descale_strides, rotary_cos, rotary_sin,
                          rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot, q_strides, H, N_q,
                          per_row, B, H_kv, N_new, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum, hip_stream};
    Fa2AppendProblem p;
    const int rc = check_append(a, p);
    if (rc != FA2_OK) return rc;
    // the attention reads the rotated Q (contiguous; p.Q null: no tables, Q as it is) and the new lengths
    const int64_t rot_strides[4] = {(int64_t)H * N_q * d, (int64_t)N_q * d, d, 1};
    DecodeCall c;
    c.Q = p.Q ? q_rot : Q; c.K = K; c.V = V; c.O = O; c.L = L; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = p.Q ? rot_strides : q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = o_strides;
    c.l_strides = l_strides; c.cache_seqlens = seqlens_out;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    return decode(c, &p);
}

int fa2_kvcache_append_varlen(void *K, void *V, const int64_t k_strides[4], const int64_t v_strides[4], const int32_t *block_table,
                              int64_t block_table_stride, const void *k_new, const void *v_new, const int64_t k_new_strides[3],
                              const int64_t v_new_strides[3], const int32_t *cu_seqlens_new, const int32_t *cache_seqlens,
                              int32_t *seqlens_out, const float *k_descale, const float *v_descale, const int64_t k_descale_strides[2],
                              const int64_t v_descale_strides[2], const void *rotary_cos, const void *rotary_sin,
                              int64_t rotary_cos_stride, int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim,
                              int32_t rotary_interleaved, const void *Q, void *q_rot, const int64_t q_strides[3], int32_t H,
                              int32_t q_pos_per_row, int32_t B, int32_t H_kv, int32_t total_new, int32_t max_seqlen_new, int32_t S_k,
                              int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t dtype_enum,
                              int32_t kv_dtype_enum, void *hip_stream) {
    int64_t kns[4], vns[4], qs[4];
    AppendCall c = {K, V, k_strides, v_strides, block_table, block_table_stride, k_new, v_new, packed4(k_new_strides, kns),
                    packed4(v_new_strides, vns), cache_seqlens, seqlens_out, k_descale, v_descale, k_descale_strides, v_descale_strides,
                    rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot,
                    packed4(q_strides, qs), H, 0, q_pos_per_row, B, H_kv, 0, S_k, num_blocks, page_size, max_blocks, d, dtype_enum,
                    kv_dtype_enum, hip_stream};
    c.packed = true; c.cu_seqlens_new = cu_seqlens_new; c.total_new = total_new; c.max_seqlen_new = max_seqlen_new;
    Fa2AppendProblem p;
    const int rc = check_append(c, p);
    return rc != FA2_OK ? rc : fa2_launch_decode_append(p);
}

int fa2_fwd_kvcache_varlen_append(const void *Q, void *K, void *V, void *O, void *L, const int64_t q_strides[3],
                                  const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[3],
                                  int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cache_seqlens, int32_t *seqlens_out,
                                  const int32_t *block_table, int64_t block_table_stride, const float *k_descale, const float *v_descale,
                                  const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], const void *k_new,
                                  const void *v_new, const int64_t k_new_strides[3], const int64_t v_new_strides[3],
                                  const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                                  int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, void *q_rot, int32_t B, int32_t H,
                                  int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size,
                                  int32_t max_blocks, int32_t d, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale,
                                  int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes,
                                  int32_t variant, void *hip_stream) {
    const int32_t per_row = causal || window_left >= 0 || window_right >= 0;  // the fixed fused call's rule
    int64_t kns[4], vns[4], qs[4], os[4];
    AppendCall a = {K, V, k_strides, v_strides, block_table, block_table_stride, k_new, v_new, packed4(k_new_strides, kns),
                    packed4(v_new_strides, vns), cache_seqlens, seqlens_out, k_descale, v_descale, k_descale_strides, v_descale_strides,
                    rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot,
                    packed4(q_strides, qs), H, 0, per_row, B, H_kv, 0, S_k, num_blocks, page_size, max_blocks, d, dtype_enum,
                    kv_dtype_enum, hip_stream};
    a.packed = true; a.cu_seqlens_new = cu_seqlens_q; a.total_new = total_q; a.max_seqlen_new = max_seqlen_q;
    Fa2AppendProblem p;
    const int rc = check_append(a, p);
    if (rc != FA2_OK) return rc;
    // the attention reads the rotated Q (packed, contiguous; p.Q null: no tables, Q as it is) and the new lengths
    const int64_t rot_strides[4] = {0, d, (int64_t)H * d, 1}, ls[2] = {0, l_head_stride};
    DecodeCall c;
    c.Q = p.Q ? q_rot : Q; c.K = K; c.V = V; c.O = O; c.L = L; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = p.Q ? rot_strides : a.q_strides; c.k_strides = k_strides; c.v_strides = v_strides; c.o_strides = packed4(o_strides, os);
    c.l_strides = ls; c.cache_seqlens = seqlens_out;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = max_seqlen_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = k_descale; c.v_descale = v_descale; c.k_descale_strides = k_descale_strides; c.v_descale_strides = v_descale_strides;
    c.packed = true; c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    return decode(c, &p);
}

int fa2_kvcache_mla_append(void *KV, const int64_t kv_strides[4], const int32_t *block_table, int64_t block_table_stride,
                           const void *c_new, const void *pe_new, const int64_t c_new_strides[4], const int64_t pe_new_strides[4],
                           const int32_t *cache_seqlens, int32_t *seqlens_out, const float *kv_descale,
                           const int64_t kv_descale_strides[2], const void *rotary_cos, const void *rotary_sin,
                           int64_t rotary_cos_stride, int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim,
                           int32_t rotary_interleaved, const void *Q, void *q_rot, const int64_t q_strides[4], int32_t H, int32_t N_q,
                           int32_t q_pos_per_row, int32_t B, int32_t H_kv, int32_t N_new, int32_t S_k, int32_t num_blocks,
                           int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum,
                           void *hip_stream) {
    AppendCall c = {KV, nullptr, kv_strides, nullptr, block_table, block_table_stride, c_new, pe_new, c_new_strides, pe_new_strides,
                    cache_seqlens, seqlens_out, kv_descale, nullptr, kv_descale_strides, nullptr, rotary_cos, rotary_sin,
                    rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot, q_strides, H, N_q,
                    q_pos_per_row, B, H_kv, N_new, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum, hip_stream};
    c.mla = true; c.d_v = d_v;
    Fa2AppendProblem p;
    const int rc = check_append(c, p);
    return rc != FA2_OK ? rc : fa2_launch_decode_append(p);
}

int fa2_kvcache_mla_append_varlen(void *KV, const int64_t kv_strides[4], const int32_t *block_table, int64_t block_table_stride,
                                  const void *c_new, const void *pe_new, const int64_t c_new_strides[3],
                                  const int64_t pe_new_strides[3], const int32_t *cu_seqlens_new, const int32_t *cache_seqlens,
                                  int32_t *seqlens_out, const float *kv_descale, const int64_t kv_descale_strides[2],
                                  const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                                  int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, const void *Q, void *q_rot,
                                  const int64_t q_strides[3], int32_t H, int32_t q_pos_per_row, int32_t B, int32_t H_kv,
                                  int32_t total_new, int32_t max_seqlen_new, int32_t S_k, int32_t num_blocks, int32_t page_size,
                                  int32_t max_blocks, int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum,
                                  void *hip_stream) {
    int64_t cns[4], pns[4], qs[4];
    AppendCall c = {KV, nullptr, kv_strides, nullptr, block_table, block_table_stride, c_new, pe_new, packed4(c_new_strides, cns),
                    packed4(pe_new_strides, pns), cache_seqlens, seqlens_out, kv_descale, nullptr, kv_descale_strides, nullptr,
                    rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot,
                    packed4(q_strides, qs), H, 0, q_pos_per_row, B, H_kv, 0, S_k, num_blocks, page_size, max_blocks, d, dtype_enum,
                    kv_dtype_enum, hip_stream};
    c.packed = true; c.cu_seqlens_new = cu_seqlens_new; c.total_new = total_new; c.max_seqlen_new = max_seqlen_new;
    c.mla = true; c.d_v = d_v;
    Fa2AppendProblem p;
    const int rc = check_append(c, p);
    return rc != FA2_OK ? rc : fa2_launch_decode_append(p);
}

int fa2_fwd_kvcache_mla_append(const void *Q, void *KV, void *O, void *L, const int64_t q_strides[4], const int64_t kv_strides[4],
                               const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                               int32_t *seqlens_out, const int32_t *block_table, int64_t block_table_stride, const float *kv_descale,
                               const int64_t kv_descale_strides[2], const void *c_new, const void *pe_new,
                               const int64_t c_new_strides[4], const int64_t pe_new_strides[4], const void *rotary_cos,
                               const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride, int32_t S_rot,
                               int32_t rotary_dim, int32_t rotary_interleaved, void *q_rot, int32_t B, int32_t H, int32_t H_kv,
                               int32_t N_q, int32_t N_new, int32_t S_k, int32_t num_blocks, int32_t page_size, int32_t max_blocks,
                               int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale,
                               int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes,
                               int32_t variant, void *hip_stream) {
    const int32_t per_row = causal || window_left >= 0 || window_right >= 0;  // the fused call's rule for Q's rotary positions
    AppendCall a = {KV, nullptr, kv_strides, nullptr, block_table, block_table_stride, c_new, pe_new, c_new_strides, pe_new_strides,
                    cache_seqlens, seqlens_out, kv_descale, nullptr, kv_descale_strides, nullptr, rotary_cos, rotary_sin,
                    rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot, q_strides, H, N_q,
                    per_row, B, H_kv, N_new, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum, hip_stream};
    a.mla = true; a.d_v = d_v;
    Fa2AppendProblem p;
    const int rc = check_append(a, p);
    if (rc != FA2_OK) return rc;
    // the attention reads the rotated Q (contiguous; p.Q null: no tables, Q as it is), the new lengths, and V as the first d_v
    // columns of the row it scores: the one descale is K's and V's
    const int64_t rot_strides[4] = {(int64_t)H * N_q * d, (int64_t)N_q * d, d, 1};
    DecodeCall c;
    c.Q = p.Q ? q_rot : Q; c.K = KV; c.V = KV; c.O = O; c.L = L; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = p.Q ? rot_strides : q_strides; c.k_strides = kv_strides; c.v_strides = kv_strides; c.o_strides = o_strides;
    c.l_strides = l_strides; c.cache_seqlens = seqlens_out;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = N_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = kv_descale; c.v_descale = kv_descale; c.k_descale_strides = kv_descale_strides; c.v_descale_strides = kv_descale_strides;
    return decode(c, &p);
}

int fa2_fwd_kvcache_mla_varlen_append(const void *Q, void *KV, void *O, void *L, const int64_t q_strides[3], const int64_t kv_strides[4],
                                      const int64_t o_strides[3], int64_t l_head_stride, const int32_t *cu_seqlens_q,
                                      const int32_t *cache_seqlens, int32_t *seqlens_out, const int32_t *block_table,
                                      int64_t block_table_stride, const float *kv_descale, const int64_t kv_descale_strides[2],
                                      const void *c_new, const void *pe_new, const int64_t c_new_strides[3],
                                      const int64_t pe_new_strides[3], const void *rotary_cos, const void *rotary_sin,
                                      int64_t rotary_cos_stride, int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim,
                                      int32_t rotary_interleaved, void *q_rot, int32_t B, int32_t H, int32_t H_kv, int32_t total_q,
                                      int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size, int32_t max_blocks,
                                      int32_t d, int32_t d_v, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale,
                                      int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace,
                                      int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    const int32_t per_row = causal || window_left >= 0 || window_right >= 0;  // the fused call's rule for Q's rotary positions
    int64_t cns[4], pns[4], qs[4], os[4];
    AppendCall a = {KV, nullptr, kv_strides, nullptr, block_table, block_table_stride, c_new, pe_new, packed4(c_new_strides, cns),
                    packed4(pe_new_strides, pns), cache_seqlens, seqlens_out, kv_descale, nullptr, kv_descale_strides, nullptr,
                    rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot,
                    packed4(q_strides, qs), H, 0, per_row, B, H_kv, 0, S_k, num_blocks, page_size, max_blocks, d, dtype_enum,
                    kv_dtype_enum, hip_stream};
    a.packed = true; a.cu_seqlens_new = cu_seqlens_q; a.total_new = total_q; a.max_seqlen_new = max_seqlen_q;
    a.mla = true; a.d_v = d_v;
    Fa2AppendProblem p;
    const int rc = check_append(a, p);
    if (rc != FA2_OK) return rc;
    // the attention reads the rotated Q (packed, contiguous; p.Q null: no tables, Q as it is), the new lengths, and V as the first d_v
    // columns of the row it scores: the one descale is K's and V's
    const int64_t rot_strides[4] = {0, d, (int64_t)H * d, 1}, ls[2] = {0, l_head_stride};
    DecodeCall c;
    c.Q = p.Q ? q_rot : Q; c.K = KV; c.V = KV; c.O = O; c.L = L; c.variant = variant; c.hip_stream = hip_stream;
    c.q_strides = p.Q ? rot_strides : a.q_strides; c.k_strides = kv_strides; c.v_strides = kv_strides; c.o_strides = packed4(o_strides, os);
    c.l_strides = ls; c.cache_seqlens = seqlens_out;
    c.B = B; c.H = H; c.H_kv = H_kv; c.N_q = max_seqlen_q; c.S_k = S_k; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale;
    c.window_left = window_left; c.window_right = window_right; c.num_splits = num_splits; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.mla = true; c.d_v = d_v;
    c.block_table = block_table; c.block_table_stride = block_table_stride; c.num_blocks = num_blocks; c.page_size = page_size; c.max_blocks = max_blocks;
    c.fp8 = kv_dtype_enum != dtype_enum; c.kv_dtype_enum = kv_dtype_enum;
    c.k_descale = kv_descale; c.v_descale = kv_descale; c.k_descale_strides = kv_descale_strides; c.v_descale_strides = kv_descale_strides;
    c.packed = true; c.cu_seqlens_q = cu_seqlens_q; c.total_q = total_q; c.max_seqlen_q = max_seqlen_q;
    return decode(c, &p);
}

}  // extern "C"
