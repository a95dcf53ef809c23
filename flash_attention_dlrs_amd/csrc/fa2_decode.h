// Shared declarations of the KV-cache decode kernels (fa2_fwd_kvcache, include/fa2_fwd.h): internal.
#pragma once
#include "fa2_common.h"

// Split granularity: split s of sequence b covers keys [s c, (s + 1) c) with c = ceil(N_k(b) / num_splits) rounded up to this.
#define FA2_KVCACHE_KEY_TILE 64

// One decode problem as fa2_fwd_kvcache hands it over, arguments already checked.  Strides in elements of each tensor's dtype.
struct Fa2DecodeProblem {
    const void *Q, *K, *V;
    void *O, *L;
    int64_t qs[4], ks[4], vs[4], os[4], ls[2];
    const int32_t *seqlens;  // device, B entries, or null (N_k = S_k)
    int32_t B, H, H_kv, N_q, S_k, d;
    // value head size (fa2_fwd_kvcache_mla): V is (B, H_kv, S_k, d_v), O and the partials have d_v columns.  Every other entry
    // point sets d_v = d.  V may overlap K in memory (MLA: V = K[..., :d_v]); neither is written.
    int32_t d_v;
    int32_t dtype, causal;
    // fp8 KV cache (fa2_fwd_kvcache_fp8): kv_dtype is the element type of K and V (== dtype otherwise), kd / vd the device
    // descales at [b * s[0] + h_kv * s[1]], null = 1.  K = kd * float(K8), V = vd * float(V8).
    int32_t kv_dtype;
    const float *kd, *vd;
    int64_t kds[2], vds[2];
    // paged cache (fa2_fwd_kvcache_paged): table non-null.  K, V are the page pool (num_blocks, H_kv, page_size, d), ks[0] / vs[0] the
    // block stride, S_k the capacity max_blocks * page_size; key j of sequence b is row j % page_size of page
    // table[b * table_stride + j / page_size], the entry clamped to [0, num_blocks - 1] by the kernel that reads it.
    const int32_t *table;
    int64_t table_stride;
    int32_t page_size, num_blocks;
    int32_t wl, wr;  // raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    float scale;
    int32_t num_splits;  // resolved, >= 1
    float *o_part;       // [num_splits][B * H * N_q][d_v]   (num_splits > 1 only)
    float *l_part;       // [num_splits][B * H * N_q]
    hipStream_t stream;
    // variable-length (packed) queries (fa2_fwd_kvcache_varlen): cu_q non-null.  Q, O are (total_q, H, d) with qs / os =
    // {0, head, token, d}, L is (H, total_q) with ls = {0, head}; sequence b owns n_q(b) = fa2_varlen_seq(cu_q, b, total_q, max_q)
    // rows from its start on, N_q holds max_q, and the partials are [num_splits][total_q * H] rows, row = token * H + head.
    const int32_t *cu_q;
    int32_t total_q, max_q;
    // per-query key lists (fa2_fwd_kvcache_mla_sparse): indices non-null.  Entry [b, h_kv, qi, s] at the element strides is[4] is a
    // key position of sequence b, no key outside [0, N_k(b)); topk slots per list, the splits run over the slots
    // (fa2_decode_split_slots), causal / wl / wr are not read.
    const int32_t *indices;
    int64_t is[4];
    int32_t topk;
};

// N_k(b) and the key range [k0, k1) of split s (device side of the rule above).
__device__ __forceinline__ void fa2_decode_split(const int32_t *seqlens, int b, int S_k, int num_splits, int s, int &nk, int &k0,
                                                 int &k1) {
    int n = seqlens ? seqlens[b] : S_k;
    n = n < 0 ? 0 : (n > S_k ? S_k : n);
    const int c = ((n + num_splits - 1) / num_splits + FA2_KVCACHE_KEY_TILE - 1) & ~(FA2_KVCACHE_KEY_TILE - 1);
    nk = n;
    k0 = s * c;  // <= n + 64 * num_splits
    k1 = k0 + c < n ? k0 + c : n;
}

// The sparse call: N_k(b) and the SLOT range [s0, s1) of split s over a list of topk slots, c = ceil(topk / num_splits) rounded up
// to the key tile.  With the identity list over N_k(b) = topk keys these are fa2_decode_split's k0, k1.
__device__ __forceinline__ void fa2_decode_split_slots(const int32_t *seqlens, int b, int S_k, int topk, int num_splits, int s, int &nk,
                                                       int &s0, int &s1) {
    const int n = seqlens ? seqlens[b] : S_k;
    nk = n < 0 ? 0 : (n > S_k ? S_k : n);
    const int c = ((topk + num_splits - 1) / num_splits + FA2_KVCACHE_KEY_TILE - 1) & ~(FA2_KVCACHE_KEY_TILE - 1);
    s0 = s * c;  // <= topk + 64 * num_splits
    s1 = s0 + c < topk ? s0 + c : topk;
}

// A descale of the fp8 cache at [b, h_kv]: uniform over the workgroup, so one scalar load.  Null = 1.
__device__ __forceinline__ float fa2_decode_descale(const float *p, int64_t s0, int64_t s1, int b, int hk) {
    return p ? p[b * s0 + hk * s1] : 1.0f;
}

// Cache element types of the matrix forms other than the I/O type T (fa2_decode_mfma16.hip, fa2_decode_mla16.hip): OCP e4m3fn and
// e5m2, one byte each.  CacheCvt<T, C>::cvt<HI>(w) converts bytes 2 HI, 2 HI + 1 of a word to a pair of T with v_cvt_scalef32_pk_*
// at scale 1.0: exactly, both formats are subsets of f16 and of bf16.
struct CacheE4M3 {};
struct CacheE5M2 {};
typedef __attribute__((ext_vector_type(2))) __bf16 fa2_bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 fa2_f16x2;
template <typename T, typename C> struct CacheCvt;
template <> struct CacheCvt<__bf16, CacheE4M3> {
    template <bool HI> static __device__ __forceinline__ unsigned cvt(unsigned w) {
        return __builtin_bit_cast(unsigned, (fa2_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
    }
};
template <> struct CacheCvt<__bf16, CacheE5M2> {
    template <bool HI> static __device__ __forceinline__ unsigned cvt(unsigned w) {
        return __builtin_bit_cast(unsigned, (fa2_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(w, 1.0f, HI));
    }
};
template <> struct CacheCvt<_Float16, CacheE4M3> {
    template <bool HI> static __device__ __forceinline__ unsigned cvt(unsigned w) {
        return __builtin_bit_cast(unsigned, (fa2_f16x2)__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
    }
};
template <> struct CacheCvt<_Float16, CacheE5M2> {
    template <bool HI> static __device__ __forceinline__ unsigned cvt(unsigned w) {
        return __builtin_bit_cast(unsigned, (fa2_f16x2)__builtin_amdgcn_cvt_scalef32_pk_f16_bf8(w, 1.0f, HI));
    }
};

// A block-table entry as the kernels use it: clamped into the pool, so a wild entry cannot become an access outside it.
__device__ __forceinline__ int fa2_decode_page(const int32_t *table, int64_t i, int num_blocks) {
    const int e = table[i];
    return e < 0 ? 0 : (e > num_blocks - 1 ? num_blocks - 1 : e);
}

bool fa2_decode_mfma16_supports(const Fa2DecodeProblem &p);
int fa2_launch_decode_mfma16(const Fa2DecodeProblem &p);
int fa2_launch_decode_generic(const Fa2DecodeProblem &p);
// The form AUTO takes as far as the shape alone decides it (strides and alignment are the call's): the split heuristic counts
// the workgroups of that form.
static inline bool fa2_decode_mfma16_shape(int32_t H, int32_t H_kv, int32_t N_q, int32_t d, int32_t dtype) {
    return (dtype == FA2_DTYPE_F16 || dtype == FA2_DTYPE_BF16) && (d == 64 || d == 128) && H_kv >= 1 &&
           (int64_t)(H / H_kv) * N_q <= 64;
}
int fa2_launch_decode_combine(const Fa2DecodeProblem &p);  // second launch, num_splits > 1 only

// The latent-cache matrix form (fa2_decode_mla16.hip, FA2_KVCACHE_VARIANT_MLA16): d = 576, d_v = 512, V the first 512 columns of K,
// 64 rows of a KV group per workgroup, ceil(g N_q / 64) row tiles per (split, KV head, sequence).
static inline bool fa2_decode_mla16_shape(int32_t d, int32_t d_v, int32_t dtype) {
    return (dtype == FA2_DTYPE_F16 || dtype == FA2_DTYPE_BF16) && d == 576 && d_v == 512;
}
bool fa2_decode_mla16_supports(const Fa2DecodeProblem &p);
int fa2_launch_decode_mla16(const Fa2DecodeProblem &p);

// The query-tiled matrix form of the packed call (fa2_decode_mfma16_v.hip): a workgroup owns tq consecutive query positions of one
// sequence for the g heads of a KV group, R = g tq <= 64 rows.
// (g in [1, 64]: the callers have checked it, the shape test below included)
static inline int32_t fa2_decode_varlen_tq(int32_t g, int32_t max_q) { return 64 / g < max_q ? 64 / g : max_q; }
// H < H_kv (no whole group: g = 0) and H % H_kv != 0 are no problem of this form: a call refuses them, the heuristic counts them
// as the VALU form's.
static inline bool fa2_decode_mfma16_v_shape(int32_t H, int32_t H_kv, int32_t d, int32_t dtype) {
    return (dtype == FA2_DTYPE_F16 || dtype == FA2_DTYPE_BF16) && (d == 64 || d == 128) && H_kv >= 1 && H >= H_kv && H % H_kv == 0 &&
           H / H_kv <= 64;
}
bool fa2_decode_mfma16_v_supports(const Fa2DecodeProblem &p);
int fa2_launch_decode_mfma16_v(const Fa2DecodeProblem &p);

// The query-tiled form of the latent-cache matrix kernel (fa2_decode_mla16_v.hip, fa2_fwd_kvcache_mla_varlen): the g n_q(b) rows of a
// (sequence, KV head) position-major, 64 of them per workgroup, ceil(g max_seqlen_q / 64) tiles per (split, KV head, sequence).
bool fa2_decode_mla16_v_supports(const Fa2DecodeProblem &p);
int fa2_launch_decode_mla16_v(const Fa2DecodeProblem &p);

// The sparse call (fa2_fwd_kvcache_mla_sparse).  Matrix form (fa2_decode_mla16_s.hip): the list-addressed instantiations of the latent
// kernel, 64 heads of one (sequence, KV head, query position) per workgroup, ceil(g / 64) head tiles.  VALU form
// (fa2_decode_sparse_generic.hip): 16 heads of one KV group at one query position per workgroup, every dtype, any d / d_v, any V.
bool fa2_decode_mla16_s_supports(const Fa2DecodeProblem &p);
int fa2_launch_decode_mla16_s(const Fa2DecodeProblem &p);
int fa2_launch_decode_sparse_generic(const Fa2DecodeProblem &p);

// The packed sparse call (fa2_fwd_kvcache_mla_sparse_varlen): cu_q AND indices non-null.  Q, O, L and the partials are the packed
// call's (above), is = {0, KV head, token, slot}: entry [t, h_kv, s] is a key position of the sequence that owns packed row t
// (fa2_varlen_owner).  The grids run over total_q tokens in B * N_q's place; a workgroup whose row no sequence owns leaves at once and
// writes nothing, as the combine (which walks the sequences' own rows) then reads and writes nothing of it.  The packed instantiations
// of both forms, a translation unit each (fa2_decode_mla16_sv.hip, fa2_decode_sparse_generic_v.hip).
bool fa2_decode_mla16_sv_supports(const Fa2DecodeProblem &p);
int fa2_launch_decode_mla16_sv(const Fa2DecodeProblem &p);
int fa2_launch_decode_sparse_generic_v(const Fa2DecodeProblem &p);

// One cache append as fa2_kvcache_append hands it over (fa2_decode_append.hip), arguments already checked.  Strides in elements of
// each tensor's dtype.  It is the kernel's argument as well.
struct Fa2AppendProblem {
    void *K, *V;  // the cache (B, H_kv, capacity, d) or, with `table`, the page pool (num_blocks, H_kv, page_size, d)
    int64_t ks[4], vs[4];
    const int32_t *table;  // as in Fa2DecodeProblem, or null
    int64_t table_stride;
    int32_t page_size, num_blocks;
    int32_t capacity;  // S_k, or max_blocks * page_size
    const void *k_new, *v_new;  // (B, H_kv, N_new, d) in `dtype`
    int64_t kns[4], vns[4];
    const int32_t *seqlens;  // device, B entries: token t of sequence b becomes key clamp(seqlens[b], 0, capacity) + t
    int32_t *seqlens_out;    // device, B entries: min(clamp(seqlens[b], 0, capacity) + N_new, capacity)
    const float *kd, *vd;    // fp8 cache: the stored byte is fp8(x / descale); null = 1
    int64_t kds[2], vds[2];
    const void *cos, *sin;  // (S_rot, rotary_dim / 2) in `dtype`, unit last stride, or both null: no rotary
    int64_t cos_stride, sin_stride;
    int32_t S_rot, rotary_dim, interleaved;
    const void *Q;  // (B, H, N_q, d), rotated into q_rot (contiguous) when the tables are given; null: the cache alone
    void *q_rot;
    int64_t qs[4];
    int32_t H, N_q, q_pos_per_row;
    int32_t B, H_kv, N_new, d;
    int32_t dtype, kv_dtype;
    hipStream_t stream;
    // packed (ragged) tokens (fa2_kvcache_append_varlen): cu_new non-null.  k_new, v_new are (total_new, H_kv, d) and Q, q_rot
    // (total_new, H, d), all over cu_new, with kns / vns / qs = {0, head, token, d}; sequence b brings the n_new(b) rows
    // fa2_varlen_seq(cu_new, b, total_new, max_new) gives it, row i of them becomes key clamp(seqlens[b], 0, capacity) + i, and
    // seqlens_out[b] = min(clamp(seqlens[b], 0, capacity) + n_new(b), capacity).  N_new and N_q are not read.  Offsets that are not
    // non-decreasing may put wrong rows into the cache; every address formed is still inside the tensors: a packed row t is
    // < total_new, its sequence b is in [0, B), its key index is < capacity, pages and positions are clamped as always.
    const int32_t *cu_new;
    int32_t total_new, max_new;
    // the latent form (fa2_kvcache_mla_append, fa2_kvcache_mla_append_varlen): V null.  K is the one tensor of an MLA cache, rows of
    // d columns whose first d_v are the value; k_new / kns are c_new, the columns [0, d_v) of a new row, pe_new / pns (shaped and
    // strided like k_new) its columns [d_v, d), and the rotary range is [d_v, d_v + rotary_dim) -- in Q too.  kd is the row's one
    // descale; v_new, vs, vns, vd are not read.  The other forms do not read these three.
    const void *pe_new;
    int64_t pns[4];
    int32_t d_v;
};
int fa2_launch_decode_append(const Fa2AppendProblem &p);
