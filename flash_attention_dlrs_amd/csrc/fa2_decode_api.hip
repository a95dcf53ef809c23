// fa2_decode_api.hip -- extern "C" entry points of KV-cache decode attention (fa2_fwd_kvcache, fa2_fwd_kvcache_fp8,
// fa2_fwd_kvcache_paged, the latent-cache call fa2_fwd_kvcache_mla, the packed-query call fa2_fwd_kvcache_varlen, the cache appends fa2_kvcache_append and fa2_kvcache_append_varlen,
// the fused steps fa2_fwd_kvcache_append and fa2_fwd_kvcache_varlen_append, and their helpers, declared in
// include/fa2_fwd.h): argument checks before any launch, the split heuristic, the choice between the two kernel forms, and the
// launches (the append where asked for, the split kernels, then the combine) on the caller's stream.
#include "fa2_decode.h"

namespace {

// fa2_kvcache_num_splits: enough splits to put kSplitWaves x 256 workgroups on the chip, every split at least kMinSplitTiles key
// tiles long (judged on the capacity: the lengths live on the device).  `base` is the workgroup count of the unsplit launch of
// the form AUTO takes for the shape: B * H_kv for the matrix form, B * H * ceil(N_q / 16) for the VALU form.  The constants are
// read off the num_splits sweep of benchmarks/bench_decode.py ("Decode attention").
constexpr int kChipWorkgroups = 256;  // one per CU
constexpr int kSplitWaves = 2;
constexpr int kMinSplitTiles = 4;
constexpr int64_t kMaxRows = 1LL << 40;  // B * H * N_q beyond this is refused: the workspace size stays far inside int64

int num_splits_auto(int64_t B, int64_t H, int64_t H_kv, int64_t N_q, int64_t S_k, int32_t d, int32_t dtype) {
    const int64_t base = fa2_decode_mfma16_shape((int32_t)H, (int32_t)H_kv, (int32_t)N_q, d, dtype) ? B * H_kv
                                                                                                     : B * H * ((N_q + 15) / 16);
    if (base >= kChipWorkgroups) return 1;
    int64_t n = (kSplitWaves * kChipWorkgroups + base - 1) / base;
    const int64_t tiles = (S_k + FA2_KVCACHE_KEY_TILE - 1) / FA2_KVCACHE_KEY_TILE;
    const int64_t cap = tiles / kMinSplitTiles;
    if (n > cap) n = cap;
    if (n > FA2_KVCACHE_MAX_SPLITS) n = FA2_KVCACHE_MAX_SPLITS;
    return n < 1 ? 1 : (int)n;
}

// fa2_kvcache_mla_num_splits: the same rule for fa2_fwd_kvcache_mla.  The latent matrix form (fa2_decode_mla16.hip) runs ONE
// workgroup per CU (its LDS tile and registers fill it), B * H_kv * ceil(g N_q / 64) of them unsplit, so one wave of the chip is
// what the splits fill (kMlaSplitWaves), and a split is at least kMlaMinSplitTiles 64-key tiles long: each workgroup loads its
// 64 x 576 Q fragments and writes 64 x 512 fp32 partials whatever its length.  The constants are read off the split sweep of
// benchmarks/bench_mla_decode.py ("MLA decode").  Every other shape is counted as the VALU form's.
constexpr int kMlaSplitWaves = 1;
constexpr int kMlaMinSplitTiles = 4;

int num_splits_mla(int64_t B, int64_t H, int64_t H_kv, int64_t N_q, int64_t S_k, int32_t d, int32_t d_v, int32_t dtype) {
    if (!fa2_decode_mla16_shape(d, d_v, dtype) || H_kv < 1 || H % H_kv != 0) return num_splits_auto(B, H, H_kv, N_q, S_k, 0, dtype);
    const int64_t base = B * H_kv * ((H / H_kv * N_q + 63) / 64);
    if (base >= kChipWorkgroups) return 1;
    int64_t n = (kMlaSplitWaves * kChipWorkgroups + base - 1) / base;
    const int64_t cap = (S_k + FA2_KVCACHE_KEY_TILE - 1) / FA2_KVCACHE_KEY_TILE / kMlaMinSplitTiles;
    if (n > cap) n = cap;
    if (n > FA2_KVCACHE_MAX_SPLITS) n = FA2_KVCACHE_MAX_SPLITS;
    return n < 1 ? 1 : (int)n;
}

int64_t workspace_bytes(int64_t B, int64_t H, int64_t N_q, int64_t d, int64_t num_splits) {
    if (num_splits <= 1) return 0;
    if (num_splits > FA2_KVCACHE_MAX_SPLITS) num_splits = FA2_KVCACHE_MAX_SPLITS;
    const int64_t rows = B * H * N_q;  // <= 2^16 * 2^16 * 2^28
    if (rows > kMaxRows || d > 512) return INT64_MAX;  // (4 * 128 * 2^40 * 513 < 2^63)
    return 4 * num_splits * rows * (d + 1);
}

// fa2_kvcache_varlen_num_splits: the same rule with the unsplit workgroup count of the packed launch in `base`'s place.  A
// sequence fills ceil(n_q(b) / tq) query tiles, the lengths live on the device: the count is bounded by the grid,
// B * ceil(max_seqlen_q / tq), and by ceil(total_q / tq) + B (every sequence ends in at most one partly filled tile), per KV
// head of the matrix form (tq = min(64 / g, max_seqlen_q)), per query head of the VALU form (tq = 16).
int num_splits_varlen(int64_t B, int64_t H, int64_t H_kv, int64_t total_q, int64_t max_q, int64_t S_k, int32_t d, int32_t dtype) {
    const bool mfma = fa2_decode_mfma16_v_shape((int32_t)H, (int32_t)H_kv, d, dtype);
    const int64_t tq = mfma ? fa2_decode_varlen_tq((int32_t)(H / H_kv), (int32_t)max_q) : 16;
    const int64_t grid = B * ((max_q + tq - 1) / tq), packed = (total_q + tq - 1) / tq + B;
    const int64_t base = (mfma ? H_kv : H) * (grid < packed ? grid : packed);
    if (base >= kChipWorkgroups) return 1;
    int64_t n = (kSplitWaves * kChipWorkgroups + base - 1) / base;
    const int64_t cap = (S_k + FA2_KVCACHE_KEY_TILE - 1) / FA2_KVCACHE_KEY_TILE / kMinSplitTiles;
    if (n > cap) n = cap;
    if (n > FA2_KVCACHE_MAX_SPLITS) n = FA2_KVCACHE_MAX_SPLITS;
    return n < 1 ? 1 : (int)n;
}

int64_t workspace_bytes_varlen(int64_t total_q, int64_t H, int64_t d, int64_t num_splits) {
    if (num_splits <= 1) return 0;
    if (num_splits > FA2_KVCACHE_MAX_SPLITS) num_splits = FA2_KVCACHE_MAX_SPLITS;
    const int64_t rows = total_q * H;
    if (rows > kMaxRows || d > 512) return INT64_MAX;
    return 4 * num_splits * rows * (d + 1);
}

// The packed queries of fa2_fwd_kvcache_varlen, checked by it.  Null for the fixed-N_q entry points.
struct VarlenQ {
    const int32_t *cu_q;
    int32_t total_q, max_q;
};

// The descales of an fp8 cache (fa2_fwd_kvcache_fp8).  Null for the 16-bit entry points, whose cache has Q's dtype.
struct Fp8Cache {
    int32_t kv_dtype;
    const float *kd, *vd;
    const int64_t *kds, *vds;
};

// The block table of a paged cache (fa2_fwd_kvcache_paged).  Null for the contiguous entry points.
struct PagedCache {
    const int32_t *table;
    int64_t table_stride;
    int32_t num_blocks, page_size, max_blocks;
};

// S_k is the capacity of a contiguous cache; with `pg` it is ignored and max_blocks * page_size takes its place.  With `append`
// (checked by check_append) that launch goes first, once every check here has passed.  `mla_dv` non-null: fa2_fwd_kvcache_mla, V
// is (B, H_kv, S_k, *mla_dv), d may reach 576 and FA2_KVCACHE_VARIANT_MLA16 is a variant; null: every other entry point, d_v = d.
int fwd_kvcache(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4], const int64_t k_strides[4],
                const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum, int32_t causal,
                float scale, int32_t wl, int32_t wr, int32_t num_splits, void *workspace, int64_t workspace_bytes_given,
                void *hip_stream, int32_t variant, const Fp8Cache *f8 = nullptr, const PagedCache *pg = nullptr,
                const Fa2AppendProblem *append = nullptr, const VarlenQ *vq = nullptr, const int32_t *mla_dv = nullptr) {
    // (with `vq`: N_q is max_seqlen_q, the strides are {0, head, token, d} and {0, head}, all checked by the caller)
    const void *ptrs[10] = {Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides};
    const char *names[10] = {"Q", "K", "V", "O", "L", "q_strides", "k_strides", "v_strides", "o_strides", "l_strides"};
    for (int t = 0; t < 10; ++t)
        if (!ptrs[t]) {
            fa2_set_error("kvcache: null %s", names[t]);
            return FA2_ERR_BAD_ARG;
        }
    if (pg) {
        if (!pg->table) {
            fa2_set_error("kvcache paged: null block_table");
            return FA2_ERR_BAD_ARG;
        }
        if (pg->num_blocks < 1 || pg->page_size < 1 || pg->max_blocks < 1) {
            fa2_set_error("kvcache paged: num_blocks, page_size and max_blocks must be >= 1 (got num_blocks=%d, page_size=%d, "
                          "max_blocks=%d)", pg->num_blocks, pg->page_size, pg->max_blocks);
            return FA2_ERR_BAD_ARG;
        }
        const int64_t cap = (int64_t)pg->max_blocks * pg->page_size;
        if (cap > (1 << 28)) {
            fa2_set_error("kvcache paged: the capacity max_blocks * page_size must be <= 2^28 (got %lld)", (long long)cap);
            return FA2_ERR_BAD_ARG;
        }
        if (pg->table_stride < 0) {
            fa2_set_error("kvcache paged: negative block_table_stride");
            return FA2_ERR_BAD_ARG;
        }
        S_k = (int32_t)cap;
    }
    if (B < 1 || B > 65535) {
        fa2_set_error("kvcache: B must be in [1, 65535] (got %d)", B);
        return FA2_ERR_BAD_ARG;
    }
    if (H < 1 || H > 65535) {
        fa2_set_error("kvcache: H must be in [1, 65535] (got %d)", H);
        return FA2_ERR_BAD_ARG;
    }
    int rc = fa2_check_gqa(H, H_kv);
    if (rc != FA2_OK) return rc;
    if (!vq && (N_q < 1 || N_q > (1 << 28))) {
        fa2_set_error("kvcache: N_q must be in [1, 2^28] (got %d)", N_q);
        return FA2_ERR_BAD_ARG;
    }
    if (S_k < 1 || S_k > (1 << 28)) {
        fa2_set_error("kvcache: S_k must be in [1, 2^28] (got %d)", S_k);
        return FA2_ERR_BAD_ARG;
    }
    if (!vq && (int64_t)B * H * N_q > kMaxRows) {
        fa2_set_error("kvcache: B * H * N_q must be <= 2^40 (got %lld)", (long long)B * H * N_q);
        return FA2_ERR_BAD_ARG;
    }
    if (wl < -1 || wr < -1) {
        fa2_set_error("window sides must be >= -1 (-1 = unbounded), got window=(%d, %d)", wl, wr);
        return FA2_ERR_BAD_ARG;
    }
    for (int k = 0; k < 4; ++k)
        if (q_strides[k] < 0 || k_strides[k] < 0 || v_strides[k] < 0 || o_strides[k] < 0) {
            fa2_set_error("kvcache: negative strides are not supported");
            return FA2_ERR_BAD_ARG;
        }
    if (l_strides[0] < 0 || l_strides[1] < 0) {
        fa2_set_error("kvcache: negative strides are not supported (l_strides)");
        return FA2_ERR_BAD_ARG;
    }
    if (!(scale == scale)) {
        fa2_set_error("kvcache: scale is NaN");
        return FA2_ERR_BAD_ARG;
    }
    if (num_splits < 0 || num_splits > FA2_KVCACHE_MAX_SPLITS) {
        fa2_set_error("kvcache: num_splits must be in [0, %d] (0 = auto), got %d", FA2_KVCACHE_MAX_SPLITS, num_splits);
        return FA2_ERR_BAD_ARG;
    }
    if (f8) {
        if ((f8->kd && !f8->kds) || (f8->vd && !f8->vds)) {
            fa2_set_error("kvcache fp8: null %s with a non-null descale", f8->kd && !f8->kds ? "k_descale_strides" : "v_descale_strides");
            return FA2_ERR_BAD_ARG;
        }
        if ((f8->kd && (f8->kds[0] < 0 || f8->kds[1] < 0)) || (f8->vd && (f8->vds[0] < 0 || f8->vds[1] < 0))) {
            fa2_set_error("kvcache fp8: negative strides are not supported (k_descale_strides, v_descale_strides)");
            return FA2_ERR_BAD_ARG;
        }
        if (f8->kv_dtype != FA2_DTYPE_F8E4M3 && f8->kv_dtype != FA2_DTYPE_F8E5M2) {
            fa2_set_error("kvcache fp8: kv_dtype_enum %d must be FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2", f8->kv_dtype);
            return FA2_ERR_UNSUPPORTED;
        }
        if (dtype_enum != FA2_DTYPE_F16 && dtype_enum != FA2_DTYPE_BF16) {
            fa2_set_error("kvcache fp8: dtype_enum %d (Q, O, L) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16", dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
    } else if (dtype_enum == FA2_DTYPE_F8E5M2 || dtype_enum == FA2_DTYPE_F8E4M3) {
        fa2_set_error("kvcache: fp8 is not supported (e4m3fn cannot hold L = +inf)");
        return FA2_ERR_UNSUPPORTED;
    }
    if (fa2_dtype_size(dtype_enum) == 0) {
        fa2_set_error("unknown dtype enum %d", dtype_enum);
        return FA2_ERR_UNSUPPORTED;
    }
    const int32_t d_v = mla_dv ? *mla_dv : d;
    if (mla_dv) {
        if (d < 1 || d > 576) {
            fa2_set_error("kvcache mla: d=%d must be in [1, 576]", d);
            return FA2_ERR_UNSUPPORTED;
        }
        if (d_v < 1 || d_v > 512) {
            fa2_set_error("kvcache mla: d_v=%d must be in [1, 512]", d_v);
            return FA2_ERR_UNSUPPORTED;
        }
        if (variant != FA2_KVCACHE_VARIANT_AUTO && variant != FA2_KVCACHE_VARIANT_GENERIC && variant != FA2_KVCACHE_VARIANT_MLA16) {
            fa2_set_error("kvcache mla: unknown variant %d (auto 0, generic 1, mla16 3)", variant);
            return FA2_ERR_UNSUPPORTED;
        }
    } else {
        if (d < 1 || d > 512) {
            fa2_set_error("d=%d must be in [1, 512]", d);
            return FA2_ERR_UNSUPPORTED;
        }
        if (variant != FA2_KVCACHE_VARIANT_AUTO && variant != FA2_KVCACHE_VARIANT_GENERIC && variant != FA2_KVCACHE_VARIANT_MFMA16) {
            fa2_set_error("kvcache: unknown variant %d (auto 0, generic 1, mfma16 2)", variant);
            return FA2_ERR_UNSUPPORTED;
        }
    }

    Fa2DecodeProblem p;
    p.Q = Q; p.K = K; p.V = V; p.O = O; p.L = L;
    for (int k = 0; k < 4; ++k) { p.qs[k] = q_strides[k]; p.ks[k] = k_strides[k]; p.vs[k] = v_strides[k]; p.os[k] = o_strides[k]; }
    p.ls[0] = l_strides[0]; p.ls[1] = l_strides[1];
    p.seqlens = cache_seqlens;
    p.B = B; p.H = H; p.H_kv = H_kv; p.N_q = N_q; p.S_k = S_k; p.d = d; p.d_v = d_v;
    p.kv_dtype = f8 ? f8->kv_dtype : dtype_enum;
    p.kd = f8 ? f8->kd : nullptr; p.vd = f8 ? f8->vd : nullptr;
    for (int k = 0; k < 2; ++k) { p.kds[k] = p.kd ? f8->kds[k] : 0; p.vds[k] = p.vd ? f8->vds[k] : 0; }
    p.table = pg ? pg->table : nullptr;
    p.table_stride = pg ? pg->table_stride : 0;
    p.page_size = pg ? pg->page_size : 0; p.num_blocks = pg ? pg->num_blocks : 0;
    p.dtype = dtype_enum; p.causal = causal != 0; p.wl = wl; p.wr = wr; p.scale = scale;
    p.cu_q = vq ? vq->cu_q : nullptr;
    p.total_q = vq ? vq->total_q : 0; p.max_q = vq ? vq->max_q : 0;
    if (num_splits != 0) p.num_splits = num_splits;
    else if (mla_dv) p.num_splits = num_splits_mla(B, H, H_kv, N_q, S_k, d, d_v, dtype_enum);
    else p.num_splits = vq ? num_splits_varlen(B, H, H_kv, vq->total_q, vq->max_q, S_k, d, dtype_enum) : num_splits_auto(B, H, H_kv, N_q, S_k, d, dtype_enum);
    p.stream = (hipStream_t)hip_stream;
    p.o_part = nullptr; p.l_part = nullptr;
    if (p.num_splits > 1) {
        const int64_t need = vq ? workspace_bytes_varlen(vq->total_q, H, d, p.num_splits) : workspace_bytes(B, H, N_q, d_v, p.num_splits);
        if (!workspace || workspace_bytes_given < need) {
            fa2_set_error("kvcache: workspace of %lld bytes needed for num_splits=%d (%s), got %s%lld", (long long)need, p.num_splits,
                          vq ? "fa2_kvcache_varlen_workspace_bytes" : "fa2_kvcache_workspace_bytes", workspace ? "" : "null, ",
                          (long long)workspace_bytes_given);
            return FA2_ERR_BAD_ARG;
        }
        p.o_part = (float *)workspace;
        p.l_part = p.o_part + (int64_t)p.num_splits * (vq ? (int64_t)vq->total_q * H : (int64_t)B * H * N_q) * d_v;
    }
    if (mla_dv) {  // the latent-cache call: its own matrix form where it runs, else the VALU form; the same combine
        if (variant == FA2_KVCACHE_VARIANT_AUTO)
            variant = fa2_decode_mla16_supports(p) ? FA2_KVCACHE_VARIANT_MLA16 : FA2_KVCACHE_VARIANT_GENERIC;
        rc = variant == FA2_KVCACHE_VARIANT_MLA16 ? fa2_launch_decode_mla16(p) : fa2_launch_decode_generic(p);
        if (rc != FA2_OK || p.num_splits == 1) return rc;
        return fa2_launch_decode_combine(p);
    }
    if (vq) {  // the packed call: its own matrix form (query-tiled), the same VALU form and combine
        if (variant == FA2_KVCACHE_VARIANT_AUTO)
            variant = fa2_decode_mfma16_v_supports(p) ? FA2_KVCACHE_VARIANT_MFMA16 : FA2_KVCACHE_VARIANT_GENERIC;
        if (append) {  // the fused ragged step: as below
            if (variant == FA2_KVCACHE_VARIANT_MFMA16 && !fa2_decode_mfma16_v_supports(p)) return fa2_launch_decode_mfma16_v(p);
            rc = fa2_launch_decode_append(*append);
            if (rc != FA2_OK) return rc;
        }
        rc = variant == FA2_KVCACHE_VARIANT_MFMA16 ? fa2_launch_decode_mfma16_v(p) : fa2_launch_decode_generic(p);
        if (rc != FA2_OK || p.num_splits == 1) return rc;
        return fa2_launch_decode_combine(p);
    }
    if (variant == FA2_KVCACHE_VARIANT_AUTO)
        variant = fa2_decode_mfma16_supports(p) ? FA2_KVCACHE_VARIANT_MFMA16 : FA2_KVCACHE_VARIANT_GENERIC;
    if (append) {  // the fused step: the cache update first, on the same stream (a forced form that cannot run fails before it)
        if (variant == FA2_KVCACHE_VARIANT_MFMA16 && !fa2_decode_mfma16_supports(p)) return fa2_launch_decode_mfma16(p);
        rc = fa2_launch_decode_append(*append);
        if (rc != FA2_OK) return rc;
    }
    rc = variant == FA2_KVCACHE_VARIANT_MFMA16 ? fa2_launch_decode_mfma16(p) : fa2_launch_decode_generic(p);
    if (rc != FA2_OK || p.num_splits == 1) return rc;
    return fa2_launch_decode_combine(p);
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
    for (int t = 0; t < 10; ++t)
        if (!ptrs[t]) {
            fa2_set_error("kvcache append: null %s", names[t]);
            return FA2_ERR_BAD_ARG;
        }
    if (c.seqlens_out == c.cache_seqlens) {
        fa2_set_error("kvcache append: seqlens_out must not be cache_seqlens (the call does not modify its lengths)");
        return FA2_ERR_BAD_ARG;
    }
    int64_t cap = c.S_k;
    if (c.block_table) {
        if (c.num_blocks < 1 || c.page_size < 1 || c.max_blocks < 1) {
            fa2_set_error("kvcache append: num_blocks, page_size and max_blocks must be >= 1 (got num_blocks=%d, page_size=%d, "
                          "max_blocks=%d)", c.num_blocks, c.page_size, c.max_blocks);
            return FA2_ERR_BAD_ARG;
        }
        cap = (int64_t)c.max_blocks * c.page_size;
        if (cap > (1 << 28)) {
            fa2_set_error("kvcache append: the capacity max_blocks * page_size must be <= 2^28 (got %lld)", (long long)cap);
            return FA2_ERR_BAD_ARG;
        }
        if (c.block_table_stride < 0) {
            fa2_set_error("kvcache append: negative block_table_stride");
            return FA2_ERR_BAD_ARG;
        }
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
        if (c.k_strides[k] < 0 || c.v_strides[k] < 0 || c.k_new_strides[k] < 0 || c.v_new_strides[k] < 0 || (c.Q && c.q_strides[k] < 0)) {
            fa2_set_error("kvcache append: negative strides are not supported (k_strides, v_strides, k_new_strides, v_new_strides, "
                          "q_strides)");
            return FA2_ERR_BAD_ARG;
        }
    const bool wide = c.kv_dtype_enum == c.dtype_enum;  // the cache has the inputs' dtype
    if (wide) {
        if (c.k_descale || c.v_descale) {
            fa2_set_error("kvcache append: k_descale / v_descale go with an fp8 cache (kv_dtype_enum %d == dtype_enum)", c.kv_dtype_enum);
            return FA2_ERR_BAD_ARG;
        }
        if (c.dtype_enum == FA2_DTYPE_F8E5M2 || c.dtype_enum == FA2_DTYPE_F8E4M3) {
            fa2_set_error("kvcache append: dtype_enum %d: fp8 inputs are not supported (an fp8 cache takes f16 / bf16 inputs)", c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
    } else {
        if ((c.k_descale && !c.k_descale_strides) || (c.v_descale && !c.v_descale_strides)) {
            fa2_set_error("kvcache append: null %s with a non-null descale",
                          c.k_descale && !c.k_descale_strides ? "k_descale_strides" : "v_descale_strides");
            return FA2_ERR_BAD_ARG;
        }
        if ((c.k_descale && (c.k_descale_strides[0] < 0 || c.k_descale_strides[1] < 0)) ||
            (c.v_descale && (c.v_descale_strides[0] < 0 || c.v_descale_strides[1] < 0))) {
            fa2_set_error("kvcache append: negative strides are not supported (k_descale_strides, v_descale_strides)");
            return FA2_ERR_BAD_ARG;
        }
        if (c.kv_dtype_enum != FA2_DTYPE_F8E4M3 && c.kv_dtype_enum != FA2_DTYPE_F8E5M2) {
            fa2_set_error("kvcache append: kv_dtype_enum %d must be dtype_enum, FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2", c.kv_dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
        if (c.dtype_enum != FA2_DTYPE_F16 && c.dtype_enum != FA2_DTYPE_BF16) {
            fa2_set_error("kvcache append: dtype_enum %d (k_new, v_new, Q) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16 under an fp8 cache",
                          c.dtype_enum);
            return FA2_ERR_UNSUPPORTED;
        }
    }
    if (fa2_dtype_size(c.dtype_enum) == 0) {
        fa2_set_error("unknown dtype enum %d", c.dtype_enum);
        return FA2_ERR_UNSUPPORTED;
    }
    if (c.d < 1 || c.d > 512) {
        fa2_set_error("d=%d must be in [1, 512]", c.d);
        return FA2_ERR_UNSUPPORTED;
    }
    const bool rotary = c.rotary_cos || c.rotary_sin;
    if (rotary) {
        if (!c.rotary_cos || !c.rotary_sin) {
            fa2_set_error("kvcache append: rotary_cos and rotary_sin go together (null %s)", c.rotary_cos ? "rotary_sin" : "rotary_cos");
            return FA2_ERR_BAD_ARG;
        }
        if (c.rotary_dim < 2 || c.rotary_dim > c.d || (c.rotary_dim & 1)) {
            fa2_set_error("kvcache append: rotary_dim must be even and in [2, d = %d] (got %d)", c.d, c.rotary_dim);
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
    p.K = c.K; p.V = c.V;
    for (int k = 0; k < 4; ++k) {
        p.ks[k] = c.k_strides[k]; p.vs[k] = c.v_strides[k]; p.kns[k] = c.k_new_strides[k]; p.vns[k] = c.v_new_strides[k];
        p.qs[k] = c.Q ? c.q_strides[k] : 0;
    }
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

// fa2_fwd_kvcache_varlen; with `append` (packed, checked by check_append) that launch goes first.
int fwd_kvcache_varlen(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                       const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[3], int64_t l_head_stride,
                       const int32_t *cu_seqlens_q, const int32_t *cache_seqlens, const int32_t *block_table,
                       int64_t block_table_stride, const float *k_descale, const float *v_descale,
                       const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                       int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks, int32_t page_size, int32_t max_blocks,
                       int32_t d, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale, int32_t window_left,
                       int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant,
                       void *hip_stream, const Fa2AppendProblem *append = nullptr) {
    if (!q_strides || !o_strides) {
        fa2_set_error("kvcache varlen: null %s", !q_strides ? "q_strides" : "o_strides");
        return FA2_ERR_BAD_ARG;
    }
    if (!cu_seqlens_q) {
        fa2_set_error("kvcache varlen: null cu_seqlens_q");
        return FA2_ERR_BAD_ARG;
    }
    if (total_q < 1) {
        fa2_set_error("kvcache varlen: total_q must be >= 1 (got %d)", total_q);
        return FA2_ERR_BAD_ARG;
    }
    if (max_seqlen_q < 1 || max_seqlen_q > (1 << 28)) {
        fa2_set_error("kvcache varlen: max_seqlen_q must be in [1, 2^28] (got %d)", max_seqlen_q);
        return FA2_ERR_BAD_ARG;
    }
    if (H >= 1 && (int64_t)total_q * H > kMaxRows) {
        fa2_set_error("kvcache varlen: total_q * H must be <= 2^40 (got %lld)", (long long)total_q * H);
        return FA2_ERR_BAD_ARG;
    }
    if (l_head_stride < 0) {
        fa2_set_error("kvcache: negative strides are not supported (l_head_stride)");
        return FA2_ERR_BAD_ARG;
    }
    const bool wide = kv_dtype_enum == dtype_enum;  // the cache has Q's dtype: no descales
    if (wide && (k_descale || v_descale)) {
        fa2_set_error("kvcache varlen: k_descale / v_descale go with an fp8 cache (kv_dtype_enum %d == dtype_enum)", kv_dtype_enum);
        return FA2_ERR_BAD_ARG;
    }
    // the packed tensors in the fixed call's terms: no batch stride, the token axis where the query position is
    const int64_t qs[4] = {0, q_strides[1], q_strides[0], q_strides[2]}, os[4] = {0, o_strides[1], o_strides[0], o_strides[2]};
    const int64_t ls[2] = {0, l_head_stride};
    const VarlenQ vq = {cu_seqlens_q, total_q, max_seqlen_q};
    const Fp8Cache f8 = {kv_dtype_enum, k_descale, v_descale, k_descale_strides, v_descale_strides};
    const PagedCache pg = {block_table, block_table_stride, num_blocks, page_size, max_blocks};
    return fwd_kvcache(Q, K, V, O, L, qs, k_strides, v_strides, os, ls, cache_seqlens, B, H, H_kv, max_seqlen_q, S_k, d, dtype_enum, causal,
                       scale, window_left, window_right, num_splits, workspace, workspace_bytes, hip_stream, variant,
                       wide ? nullptr : &f8, block_table ? &pg : nullptr, append, &vq);
}

}  // namespace

extern "C" {

int fa2_fwd_kvcache(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                    const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                    const int32_t *cache_seqlens, int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d,
                    int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                    void *workspace, int64_t workspace_bytes, void *hip_stream) {
    return fwd_kvcache(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, cache_seqlens, B, H, H_kv, N_q, S_k, d,
                       dtype_enum, causal, scale, window_left, window_right, num_splits, workspace, workspace_bytes, hip_stream,
                       FA2_KVCACHE_VARIANT_AUTO);
}

int fa2_fwd_kvcache_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                            const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                            const int64_t l_strides[2], const int32_t *cache_seqlens, int32_t B, int32_t H, int32_t H_kv,
                            int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                            int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes,
                            void *hip_stream, int32_t variant) {
    return fwd_kvcache(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, cache_seqlens, B, H, H_kv, N_q, S_k, d,
                       dtype_enum, causal, scale, window_left, window_right, num_splits, workspace, workspace_bytes, hip_stream,
                       variant);
}

int fa2_fwd_kvcache_fp8(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                        const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                        const int32_t *cache_seqlens, const float *k_descale, const float *v_descale,
                        const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                        int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum, int32_t kv_dtype_enum, int32_t causal, float scale,
                        int32_t window_left, int32_t window_right, int32_t num_splits, void *workspace, int64_t workspace_bytes,
                        int32_t variant, void *hip_stream) {
    const Fp8Cache f8 = {kv_dtype_enum, k_descale, v_descale, k_descale_strides, v_descale_strides};
    return fwd_kvcache(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, cache_seqlens, B, H, H_kv, N_q, S_k, d,
                       dtype_enum, causal, scale, window_left, window_right, num_splits, workspace, workspace_bytes, hip_stream,
                       variant, &f8);
}

int fa2_fwd_kvcache_paged(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                          const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                          const int64_t l_strides[2], const int32_t *cache_seqlens, const int32_t *block_table,
                          int64_t block_table_stride, const float *k_descale, const float *v_descale,
                          const int64_t k_descale_strides[2], const int64_t v_descale_strides[2], int32_t B, int32_t H, int32_t H_kv,
                          int32_t N_q, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t dtype_enum,
                          int32_t kv_dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                          int32_t num_splits, void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    const bool wide = kv_dtype_enum == dtype_enum;  // the pool has Q's dtype: fa2_fwd_kvcache's checks, no descales
    if (wide && (k_descale || v_descale)) {
        fa2_set_error("kvcache paged: k_descale / v_descale go with an fp8 pool (kv_dtype_enum %d == dtype_enum)", kv_dtype_enum);
        return FA2_ERR_BAD_ARG;
    }
    const Fp8Cache f8 = {kv_dtype_enum, k_descale, v_descale, k_descale_strides, v_descale_strides};
    const PagedCache pg = {block_table, block_table_stride, num_blocks, page_size, max_blocks};
    return fwd_kvcache(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, cache_seqlens, B, H, H_kv, N_q, 0, d,
                       dtype_enum, causal, scale, window_left, window_right, num_splits, workspace, workspace_bytes, hip_stream,
                       variant, wide ? nullptr : &f8, &pg);
}

int fa2_fwd_kvcache_mla(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                        const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                        const int32_t *cache_seqlens, const int32_t *block_table, int64_t block_table_stride, int32_t B, int32_t H,
                        int32_t H_kv, int32_t N_q, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                        int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                        void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream) {
    // block_table null: the contiguous cache (B, H_kv, S_k, d), a pool of one page per sequence: page_size carries S_k
    // (num_blocks and max_blocks are not read)
    const PagedCache pg = {block_table, block_table_stride, num_blocks, page_size, max_blocks};
    return fwd_kvcache(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, cache_seqlens, B, H, H_kv, N_q,
                       block_table ? 0 : page_size, d, dtype_enum, causal, scale, window_left, window_right, num_splits, workspace,
                       workspace_bytes, hip_stream, variant, nullptr, block_table ? &pg : nullptr, nullptr, nullptr, &d_v);
}

int32_t fa2_kvcache_mla_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t d_v,
                                   int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || N_q < 1 || S_k < 1) return 1;
    return num_splits_mla(B, H, H_kv, N_q, S_k, d, d_v, dtype_enum);
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
    return fwd_kvcache_varlen(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_head_stride, cu_seqlens_q, cache_seqlens,
                              block_table, block_table_stride, k_descale, v_descale, k_descale_strides, v_descale_strides, B, H, H_kv,
                              total_q, max_seqlen_q, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum, causal, scale,
                              window_left, window_right, num_splits, workspace, workspace_bytes, variant, hip_stream);
}

int64_t fa2_kvcache_varlen_workspace_bytes(int32_t total_q, int32_t H, int32_t d, int32_t num_splits) {
    if (total_q < 1 || H < 1 || d < 1 || H > 65535) return 0;
    return workspace_bytes_varlen(total_q, H, d, num_splits);
}

int32_t fa2_kvcache_varlen_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t d,
                                      int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || total_q < 1 || max_seqlen_q < 1 || S_k < 1) return 1;
    return num_splits_varlen(B, H, H_kv, total_q, max_seqlen_q, S_k, d, dtype_enum);
}

int64_t fa2_kvcache_workspace_bytes(int32_t B, int32_t H, int32_t N_q, int32_t d, int32_t num_splits) {
    if (B < 1 || H < 1 || N_q < 1 || d < 1 || B > 65535 || H > 65535 || N_q > (1 << 28)) return 0;
    return workspace_bytes(B, H, N_q, d, num_splits);
}

int32_t fa2_kvcache_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum) {
    if (B < 1 || H < 1 || H_kv < 1 || N_q < 1 || S_k < 1) return 1;
    return num_splits_auto(B, H, H_kv, N_q, S_k, d, dtype_enum);
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
    const AppendCall c = {K, V, k_strides, v_strides, block_table, block_table_stride, k_new, v_new, k_new_strides, v_new_strides,
                          cache_seqlens, seqlens_out, k_descale, v_descale, k_descale_strides, v_descale_strides, rotary_cos, rotary_sin,
                          rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot, q_strides, H, N_q,
                          per_row, B, H_kv, N_new, S_k, num_blocks, page_size, max_blocks, d, dtype_enum, kv_dtype_enum, hip_stream};
    Fa2AppendProblem p;
    const int rc = check_append(c, p);
    if (rc != FA2_OK) return rc;
    // the attention reads the rotated Q (contiguous) and the new lengths
    const int64_t rot_strides[4] = {(int64_t)H * N_q * d, (int64_t)N_q * d, d, 1};
    const bool rotated = p.Q != nullptr;
    const Fp8Cache f8 = {kv_dtype_enum, k_descale, v_descale, k_descale_strides, v_descale_strides};
    const PagedCache pg = {block_table, block_table_stride, num_blocks, page_size, max_blocks};
    return fwd_kvcache(rotated ? q_rot : Q, K, V, O, L, rotated ? rot_strides : q_strides, k_strides, v_strides, o_strides, l_strides,
                       seqlens_out, B, H, H_kv, N_q, S_k, d, dtype_enum, causal, scale, window_left, window_right, num_splits, workspace,
                       workspace_bytes, hip_stream, variant, kv_dtype_enum == dtype_enum ? nullptr : &f8, block_table ? &pg : nullptr,
                       &p);
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
    int64_t kns[4], vns[4], qs[4];
    AppendCall c = {K, V, k_strides, v_strides, block_table, block_table_stride, k_new, v_new, packed4(k_new_strides, kns),
                    packed4(v_new_strides, vns), cache_seqlens, seqlens_out, k_descale, v_descale, k_descale_strides, v_descale_strides,
                    rotary_cos, rotary_sin, rotary_cos_stride, rotary_sin_stride, S_rot, rotary_dim, rotary_interleaved, Q, q_rot,
                    packed4(q_strides, qs), H, 0, per_row, B, H_kv, 0, S_k, num_blocks, page_size, max_blocks, d, dtype_enum,
                    kv_dtype_enum, hip_stream};
    c.packed = true; c.cu_seqlens_new = cu_seqlens_q; c.total_new = total_q; c.max_seqlen_new = max_seqlen_q;
    Fa2AppendProblem p;
    const int rc = check_append(c, p);
    if (rc != FA2_OK) return rc;
    // the attention reads the rotated Q (packed, contiguous) and the new lengths
    const int64_t rot_strides[3] = {(int64_t)H * d, d, 1};
    const bool rotated = p.Q != nullptr;
    return fwd_kvcache_varlen(rotated ? q_rot : Q, K, V, O, L, rotated ? rot_strides : q_strides, k_strides, v_strides, o_strides,
                              l_head_stride, cu_seqlens_q, seqlens_out, block_table, block_table_stride, k_descale, v_descale,
                              k_descale_strides, v_descale_strides, B, H, H_kv, total_q, max_seqlen_q, S_k, num_blocks, page_size,
                              max_blocks, d, dtype_enum, kv_dtype_enum, causal, scale, window_left, window_right, num_splits, workspace,
                              workspace_bytes, variant, hip_stream, &p);
}

}  // extern "C"
