/*
 * fa2_bwd.h -- C ABI of the MI355X-native Flash-Attention-2 backward (libfa2_hip.so), SURVEY.md section 8 row f1.
 *
 * Drop-in boundary for the launch PAIR the reference's host glue makes in FlashAttention.backward
 * (src/flash_attention_torch.py:124-155; the deterministic class makes the same pair at :262-291):
 *
 *     bwd_D_kernel[grid](O, dO, D, <O strides>, <dO strides>, DB, DH, B, H, N, d, dtype)          kernels.py:115-166
 *     bwd_kernel[grid](Q, K, V, dQ, dK, dV, dO, L, D, lock_dQ, written_dQ,                        kernels.py:174-334
 *                      <Q, K, V, dQ, dK, dV, dO strides>, LB, LH, DB, DH, <lock strides>, B, H, N, d, dtype)
 *
 * fa2_bwd() takes the same tensors as plain pointers with element strides, plus the reference-preserving
 * extensions of the forward (causal, scale, stream).  What is NOT carried over: lock_dQ / written_dQ.  The
 * reference sums dQ across key-block programs through a spin lock (bwd_kernel, documented by its author as wrong on
 * first use) or an ordered hand-off that cannot complete with more than one key block (bwd_deterministic_kernel,
 * see tests/golden/gen_golden_bwd.py).  Here dK/dV and dQ come from two kernels that each own their outputs
 * (a key block per workgroup, then a query block per workgroup), so there is no cross-workgroup sum at all: the
 * result is deterministic and both reference classes (FlashAttention, FlashAttentionDeterministic) map to it.
 *
 * Ownership: the caller owns every buffer, D included: the reference's glue allocates D = empty_like(L)
 * (torch.py:105) before the launch; here D is a float32 (float64 for FA2_DTYPE_F64) scratch of 2*B*H*N elements:
 * rowsum(dO * O) kept unrounded (the reference rounds it to the I/O dtype, kernels.py:165), followed by the fp32 row
 * statistic L + log2(rowsum P) that the dQ launch measures and the dK/dV launch consumes -- the forward stores L in
 * the I/O dtype (kernels.py:108) and that rounding alone would scale a row of P by up to 2^0.125 in bf16.  Nothing is allocated, freed or
 * retained by the library; the launches are asynchronous on `hip_stream`.
 */
#ifndef FA2_BWD_H
#define FA2_BWD_H

#include <stdint.h>

#include "fa2_fwd.h" /* FA2_DTYPE_*, FA2_OK / FA2_ERR_*, fa2_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

/* Backward kernel variants (fa2_bwd_variant). */
#define FA2_BWD_VARIANT_AUTO 0
#define FA2_BWD_VARIANT_GENERIC 1 /* any dtype but fp8, any strides, d = 2^k in [16,512], any N; VALU            */
#define FA2_BWD_VARIANT_MFMA16 2  /* f16 / bf16, d in {64,128}, unit d-stride, 16-byte aligned rows; MFMA        */
#define FA2_BWD_VARIANT_MFMA32 3  /* f32 via v_mfma_f32_32x32x2_f32 (exact fp32), d in {64,128}, same layout rules */

/*
 * dQ, dK, dV = gradients of  O = softmax(scale * Q K^T [+ causal mask]) V  given dO, with P recomputed from the
 * forward's log2-domain log-sum-exp:  P = exp2(scale * log2(e) * Q K^T - L)   (kernels.py:283-285).
 *
 *   Q, K, V, O, dO : device pointers, logical shape (B, H, N, d), element strides *_strides[4]
 *   L              : (B, H, N, 1) in dtype_enum as written by fa2_fwd; l_strides = {LB, LH}, unit stride over N
 *   dQ, dK, dV     : outputs, (B, H, N, d) in dtype_enum, element strides d*_strides[4]
 *   D              : scratch, 2*B*H*N contiguous float32 (float64 if dtype_enum == FA2_DTYPE_F64), see above
 *   fp8 dtypes are rejected with FA2_ERR_UNSUPPORTED (the reference maps float8_e5m2 but its backward cannot
 *   represent the gradients in it either).
 */
int fa2_bwd(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
            void *dQ, void *dK, void *dV, void *D,
            const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
            const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4],
            const int64_t dk_strides[4], const int64_t dv_strides[4], const int64_t l_strides[2],
            int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
            void *hip_stream);

/* Same, forcing one kernel variant (tests and bench A/B). */
int fa2_bwd_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                    void *dQ, void *dK, void *dV, void *D,
                    const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                    const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4],
                    const int64_t dk_strides[4], const int64_t dv_strides[4], const int64_t l_strides[2],
                    int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                    void *hip_stream, int32_t variant);

/* Local (sliding-window) attention: the gradients of fa2_fwd_window's O, given its L.  Same arguments as fa2_bwd /
 * fa2_bwd_variant plus window_left, window_right after `scale`, with the window semantics, the causal clamp
 * (window_right -> 0), the FA2_ERR_BAD_ARG for a side < -1 and the normalisation of include/fa2_fwd.h: a window that
 * reduces to plain or causal attention runs fa2_bwd's own path.  Variants that take a window: FA2_BWD_VARIANT_AUTO
 * (MFMA16 where it runs, else GENERIC), FA2_BWD_VARIANT_GENERIC (f64, f32, f16, bf16) and FA2_BWD_VARIANT_MFMA16; a forced
 * FA2_BWD_VARIANT_MFMA32 returns FA2_ERR_UNSUPPORTED. */
int fa2_bwd_window(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                   void *dQ, void *dK, void *dV, void *D,
                   const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                   const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4],
                   const int64_t dk_strides[4], const int64_t dv_strides[4], const int64_t l_strides[2],
                   int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                   int32_t window_left, int32_t window_right, void *hip_stream);

int fa2_bwd_window_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO,
                           const void *L, void *dQ, void *dK, void *dV, void *D,
                           const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                           const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4],
                           const int64_t dk_strides[4], const int64_t dv_strides[4], const int64_t l_strides[2],
                           int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                           float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                           int32_t variant);

/* Variable-length (packed) attention: the gradients of fa2_fwd_varlen's O, given its L.  Layout, offsets, masks, empty
 * rows, argument checks and the clamping of cu_seqlens as in include/fa2_fwd.h; dQ is laid out like Q, dK / dV like K / V
 * (3-element strides {token, head, dim}).  D is a contiguous scratch of 2 * H * total_q float32 (float64 for f64).  Rows
 * without a visible key get dQ = 0 and add nothing to dK / dV; keys no query sees get dK = dV = 0.  Tokens outside every
 * sequence (cu_seqlens[B] < total, or gaps between sequences) are not written in dQ / dK / dV, as in the forward's O.
 * Deterministic, no atomics.  Variants: FA2_BWD_VARIANT_AUTO (MFMA16 where it runs, else GENERIC), FA2_BWD_VARIANT_GENERIC
 * (f64, f32, f16, bf16; d = 2^k in [16, 512], the host pads) and FA2_BWD_VARIANT_MFMA16 (f16 / bf16, d in {64, 128}, unit
 * d-stride, 16-byte aligned rows; its 32-bit offsets are judged on max_seqlen x row stride); a forced FA2_BWD_VARIANT_MFMA32
 * returns FA2_ERR_UNSUPPORTED. */
int fa2_bwd_varlen(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                   void *dQ, void *dK, void *dV, void *D,
                   const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                   const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                   const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                   const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                   int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                   int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                   void *hip_stream);

int fa2_bwd_varlen_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO,
                           const void *L, void *dQ, void *dK, void *dV, void *D,
                           const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                           const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                           const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                           const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                           int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                           int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                           int32_t window_right, void *hip_stream, int32_t variant);

/* Grouped-query (GQA) and multi-query attention: the gradients of fa2_fwd_gqa / fa2_fwd_varlen_gqa.  Arguments of fa2_bwd_window /
 * fa2_bwd_varlen (and their _variant forms) with H_kv after H.  K, V, dK and dV have H_kv heads (dense (B, H_kv, N, d), varlen
 * (total_k, H_kv, d)); Q, O, dO, L and dQ have H.  dK and dV of KV head k are the sums over query heads k g ... k g + g - 1
 * (g = H / H_kv), formed inside one workgroup per key block in a fixed order: deterministic, no atomics, no workspace.  D keeps its
 * size: 2 * B * H * N (dense), 2 * H * total_q (varlen).  FA2_ERR_BAD_ARG before any launch for H_kv < 1 or H % H_kv != 0
 * ("H_kv" in the message), plus every check of the non-GQA entry point; H_kv == H runs fa2_bwd_window(_variant) /
 * fa2_bwd_varlen(_variant) itself.  Variants: FA2_BWD_VARIANT_AUTO (MFMA16 where it runs, else GENERIC), FA2_BWD_VARIANT_GENERIC
 * (f64, f32, f16, bf16) and FA2_BWD_VARIANT_MFMA16 (f16 / bf16, d in {64, 128}); FA2_BWD_VARIANT_MFMA32 returns
 * FA2_ERR_UNSUPPORTED for H_kv < H. */
int fa2_bwd_gqa(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                void *dQ, void *dK, void *dV, void *D,
                const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4],
                const int64_t dk_strides[4], const int64_t dv_strides[4], const int64_t l_strides[2],
                int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                float scale, int32_t window_left, int32_t window_right, void *hip_stream);

int fa2_bwd_gqa_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                        void *dQ, void *dK, void *dV, void *D,
                        const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                        const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4],
                        const int64_t dk_strides[4], const int64_t dv_strides[4], const int64_t l_strides[2],
                        int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                        float scale, int32_t window_left, int32_t window_right, void *hip_stream, int32_t variant);

int fa2_bwd_varlen_gqa(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                       void *dQ, void *dK, void *dV, void *D,
                       const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                       const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                       const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                       const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t H_kv,
                       int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                       int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                       void *hip_stream);

int fa2_bwd_varlen_gqa_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO,
                               const void *L, void *dQ, void *dK, void *dV, void *D,
                               const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                               const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                               const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                               const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                               int32_t H_kv, int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                               int32_t total_k, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                               int32_t window_right, void *hip_stream, int32_t variant);

/* A value head size of its own: the gradients of fa2_fwd_varlen_dv's O, given its L (un-absorbed MLA prefill: d = 192 for Q / K,
 * d_v = 128 for V).  Arguments of fa2_bwd_varlen_gqa(_variant) with d_v after d: Q, K, dQ, dK have last axis d; V, O, dO, dV have
 * last axis d_v; L is (H, total_q) in dtype_enum as the forward stored it; D is the scratch of 2 * H * total_q float32 (float64 for
 * f64), its first half rowsum(dO * O) over the d_v columns.  Offsets and their clamping, the bottom-right causal mask and window,
 * empty rows (L = +inf: dQ row 0, the statistic stays +inf), zero-length sequences, tokens outside every sequence left unwritten in
 * all three gradients and the 64-bit per-sequence bases are fa2_bwd_varlen's; dK / dV of a KV head are summed over its query heads
 * inside one workgroup, in a fixed order.  Nothing pads a head size: d follows the forward call's rule -- d in [1, 512], with the
 * forward's codes outside it -- and not the power-of-two rule of the other backward calls; d_v outside [1, 512] is
 * FA2_ERR_BAD_ARG ("d_v" in the message), tested after every check of fa2_bwd_varlen_gqa.  The two views of one fused
 * (total, H_kv, d + d_v) buffer are a valid K and V, and a valid dK and dV.
 * Variants at d_v != d: FA2_BWD_VARIANT_AUTO (MFMA16DV where it runs, else GENERIC), FA2_BWD_VARIANT_GENERIC (f64, f32, f16, bf16;
 * any strides, any (d, d_v) in [1, 512]; VALU) and FA2_BWD_VARIANT_MFMA16DV (f16 / bf16 at exactly d 192 / d_v 128, unit d-stride,
 * row and head strides multiples of 8 elements and 16-byte aligned pointers on all eight tensors, 0 < scale < inf, and
 * (max(max_seqlen_q, max_seqlen_k) + 64) x row stride below 2 GiB on the five inputs); any other id returns FA2_ERR_UNSUPPORTED
 * with the id in the message.  At d_v == d the call IS fa2_bwd_varlen_gqa_variant -- the same kernels, the same bits -- and
 * AUTO, GENERIC and FA2_BWD_VARIANT_MFMA16 mean what they mean there. */
#define FA2_BWD_VARIANT_MFMA16DV 4 /* fa2_bwd_varlen_dv alone: f16 / bf16, d = 192 and d_v = 128; MFMA */

int fa2_bwd_varlen_dv(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                      void *dQ, void *dK, void *dV, void *D,
                      const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                      const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                      const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                      const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t H_kv,
                      int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                      int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                      void *hip_stream);

int fa2_bwd_varlen_dv_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO,
                              const void *L, void *dQ, void *dK, void *dV, void *D,
                              const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                              const int64_t o_strides[3], const int64_t do_strides[3], const int64_t dq_strides[3],
                              const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                              const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                              int32_t H_kv, int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k,
                              int32_t total_q, int32_t total_k, int32_t dtype_enum, int32_t causal, float scale,
                              int32_t window_left, int32_t window_right, void *hip_stream, int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* FA2_BWD_H */
