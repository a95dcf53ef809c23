/*
 * fa2_fwd.h -- C ABI of the MI355X-native Flash-Attention-2 forward (libfa2_hip.so).
 *
 * This is the drop-in boundary for ONE path of 17ex/flash_attention_dlrs: the Triton launch
 *
 *     fwd_kernel[grid](Q, K, V, O, L,
 *                      QB,QH,QN,Qd, KB,KH,KN,Kd, VB,VH,VN,Vd, OB,OH,ON,Od, LB,LH,
 *                      B, H, N, d, dtype)
 *
 * made at  src/flash_attention_torch.py:61-74, :201-214  and  src/flash_attention_wrappers.py:48-61
 * of the kernel defined at  src/flash_attention_kernels.py:17-109.  fa2_fwd() takes the same
 * argument list (pointers instead of torch tensors, strides in ELEMENTS exactly as the reference
 * passes them) plus the three reference-preserving extensions BASELINE.json asks for (causal,
 * scale, stream).  No torch types, no C++ types, no exceptions cross this boundary.
 *
 * Ownership: the caller owns every buffer.  O and L are allocated by the caller BEFORE the call
 * (flash_attention_torch.py:50-51); the library only writes into them, allocates nothing, and keeps
 * no pointer after returning.  The launch is asynchronous on `hip_stream`.
 * Threading: re-entrant; the only mutable state is the thread-local last-error string.
 */
#ifndef FA2_FWD_H
#define FA2_FWD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dtype_enum.  Replaces convert_triton_dtype (src/flash_attention_torch.py:7-18), which maps
 * float64 / float32 / float16 / float8_e5m2.  bf16 and OCP e4m3fn are extensions. */
#define FA2_DTYPE_F32 0
#define FA2_DTYPE_F16 1
#define FA2_DTYPE_BF16 2
#define FA2_DTYPE_F8E5M2 3
#define FA2_DTYPE_F8E4M3 4
#define FA2_DTYPE_F64 5

/* Return codes (the Python glue re-raises them as the exception classes the reference uses,
 * flash_attention_torch.py:24-32, :18). */
#define FA2_OK 0
#define FA2_ERR_BAD_ARG (-1)     /* null pointer, non-positive size, misaligned/negative stride  */
#define FA2_ERR_UNSUPPORTED (-2) /* dtype enum unknown, d outside [1, 512], or a variant that cannot run the problem */
#define FA2_ERR_BAD_N (-3)       /* N < 1                                                        */
#define FA2_ERR_LAUNCH (-4)      /* HIP reported an error at launch                              */

/* Kernel variants (fa2_fwd_variant / fa2_query_tile).  AUTO = the static gfx950 tile table that
 * replaces the reference's run-time autotuner (src/autotune_configs.py:24-201, kernels.py:11-15). */
#define FA2_VARIANT_AUTO 0
#define FA2_VARIANT_GENERIC 1 /* any dtype, any strides, any d in [1,512], any N; FMA on VALU     */
#define FA2_VARIANT_MFMA16 2  /* f16/bf16, unit d-stride; 4 waves x 32 rows.  d = 64 / 128, and every other multiple of 8  */
                              /* up to 128 with the missing columns zero-filled on load (no host padding: the        */
                              /* reference pads Q, K, V to a power of two, torch.py:38-47).  Also the fallback when  */
                              /* N * row stride does not fit 32-bit buffer offsets                                    */
#define FA2_VARIANT_MFMA16_W8 3 /* same, 8 waves x 32 rows (256-row Q tile)                        */
#define FA2_VARIANT_MFMA32 4  /* f32 via v_mfma_f32_32x32x2_f32; d = 64 / 128, other multiples of 4 up to 128 zero-filled on load */
#define FA2_VARIANT_MFMA16D 8 /* f16/bf16 software-pipelined (32-key blocks), LDS-DMA staging (buffer_load ... lds), 8 waves x 32 rows */
#define FA2_VARIANT_MFMA16D_W4 9 /* same, 4 waves x 32 rows                                          */
#define FA2_VARIANT_MFMA16H 14 /* MFMA16D with a persistent grid, next-job prefetch and a hand-ordered steady loop; 8 waves */
#define FA2_VARIANT_MFMA16H_W4 15 /* same, 4 waves x 32 rows                                          */
#define FA2_VARIANT_MFMA8X 16 /* fp8 on the double-rate v_mfma_f32_32x32x64_f8f6f4: 64-key units, 8 waves x 32 rows       */
#define FA2_VARIANT_MFMA8X_W4 17 /* same, 4 waves x 32 rows                                          */
#define FA2_VARIANT_MFMA16K 19 /* f16/bf16 small grids: 8 waves on a 128-row tile, waves w and w+4 split the KEYS and merge through LDS */
#define FA2_VARIANT_MFMA16K_R2K2 20 /* same with a 64-row tile: 2 row blocks x 2 key groups, four waves                    */
#define FA2_VARIANT_MFMA16K_R2K4 23 /* 64-row tile, 2 row blocks x 4 key groups, eight waves (d = 64)                       */
#define FA2_VARIANT_A64 24 /* f16/bf16, d = 128, N >= 256 (any): generated gfx950 assembly, 4 waves x 64 rows, one wave per SIMD */
                           /* with the whole register file (O, Q, V^T in AGPRs), persistent grid, continuous tile stream.     */
                           /* Non-finite inputs: as the reference, except that a NaN in query row q also makes row q ^ 16 of   */
                           /* the same 32-row block NaN (the row sums run on the matrix pipe, where q ^ 16's P meets a zero    */
                           /* weight); finite inputs are unaffected.                                                          */
#define FA2_VARIANT_A16 25 /* the A64 structure on the other matrix shape, v_mfma_f32_16x16x32 (the chip holds a higher clock on it):  */
                           /* same shapes, same job stream; a 64-key step is 136 MFMAs of 16 cycles instead of 72 of 32.          */
#define FA2_VARIANT_A8 26  /* OCP fp8 (e4m3fn, e5m2), d = 128, N >= 256 (causal or not): the A64 structure on the double-rate            */
                           /* v_mfma_f32_32x32x64_f8f6f4 (generated assembly, asm/fa2_a8_gen.py), P.V on its block-scaled form: the  */
                           /* running maximum is an integer and rides in P's scale operand, O is never rescaled; BASELINE configs[4]  */
#define FA2_VARIANT_A64D 27 /* f16/bf16, HEAD SIZE 64, N >= 256: the A64 kernel at d = 64 (generated assembly,                         */
                            /* asm/fa2_a64d_gen.py); causal and not                                                                  */
/* (ids 5-7, 10-13, 18 and the ablation ids belong to experimental kernels that are not part of this library:
 *  flash_attention_dlrs_amd/csrc/fa2_experiments.h, `make -C flash_attention_dlrs_amd/csrc experiments`) */

/*
 * O = softmax(scale * Q K^T [+ causal mask]) V   and   L = log2-domain log-sum-exp of the scores,
 * L = m + log2(l)  (src/flash_attention_kernels.py:105-108).  scale = 1, causal = 0 is the reference.
 *
 *   Q, K, V : device pointers, logical shape (B, H, N, d), element strides q/k/v_strides[4]
 *   O       : device pointer, (B, H, N, d), strides o_strides[4], written in dtype_enum
 *   L       : device pointer, (B, H, N, 1) in dtype_enum; l_strides = {LB, LH}; unit stride over N
 *             (kernels.py:59-65)
 *   hip_stream : hipStream_t (may be NULL = default stream)
 */
int fa2_fwd(const void *Q, const void *K, const void *V, void *O, void *L,
            const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
            const int64_t o_strides[4], const int64_t l_strides[2], int32_t B, int32_t H, int32_t N,
            int32_t d, int32_t dtype_enum, int32_t causal, float scale, void *hip_stream);

/* Same, forcing one kernel variant (tests and bench A/B).  FA2_ERR_UNSUPPORTED if the variant
 * cannot run the given problem. */
int fa2_fwd_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                    const int64_t q_strides[4], const int64_t k_strides[4],
                    const int64_t v_strides[4], const int64_t o_strides[4],
                    const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d,
                    int32_t dtype_enum, int32_t causal, float scale, void *hip_stream,
                    int32_t variant);

/*
 * Local (sliding-window) attention.  Same arguments as fa2_fwd / fa2_fwd_variant, plus the window after `scale`:
 *
 *   key j is visible to query i  iff  i - window_left <= j <= i + window_right,   a side of -1 = unbounded.
 *
 * causal != 0 also requires j <= i: window_right is clamped to 0.  Both sides must be >= -1, else FA2_ERR_BAD_ARG
 * ("window" in the message) before any launch.  O = softmax(scale * Q K^T over the visible keys) V and L the log2-domain
 * log-sum-exp over the visible keys, as fa2_fwd defines it.  Every row keeps its diagonal key, so no row is empty.
 * Normalisation: a side >= N - 1 is unbounded; then the causal clamp; a window that removes nothing beyond plain or causal
 * attention -- (-1, -1), (N-1, N-1), (-1, 0), causal with (-1, r) -- runs fa2_fwd's own path (plain, resp. causal = 1), so the
 * results are bit-identical to the plain / causal call.
 * Variants that take a window: FA2_VARIANT_AUTO (the windowed table: MFMA16D / MFMA16D_W4 where they run, else GENERIC),
 * FA2_VARIANT_GENERIC (every dtype, any strides, any d), FA2_VARIANT_MFMA16D and FA2_VARIANT_MFMA16D_W4 (f16 / bf16,
 * d in {64, 128}: blocks outside the band are skipped, blocks across its edges masked).  Any other forced variant returns
 * FA2_ERR_UNSUPPORTED for a window that does not reduce.
 */
int fa2_fwd_window(const void *Q, const void *K, const void *V, void *O, void *L,
                   const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                   const int64_t o_strides[4], const int64_t l_strides[2], int32_t B, int32_t H, int32_t N,
                   int32_t d, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                   int32_t window_right, void *hip_stream);

int fa2_fwd_window_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                           const int64_t q_strides[4], const int64_t k_strides[4],
                           const int64_t v_strides[4], const int64_t o_strides[4],
                           const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d,
                           int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                           int32_t window_right, void *hip_stream, int32_t variant);

/*
 * Variable-length (packed) attention: B sequences of different lengths in one call, as FlashAttention-2's
 * flash_attn_varlen_func takes them.
 *
 *   Layout.   Q is (total_q, H, d), K and V are (total_k, H, d), strides {token, head, dim} in elements (3 each); O is
 *             (total_q, H, d); L is (H, total_q) in the I/O dtype, unit stride over tokens, head stride l_head_stride.
 *   Offsets.  cu_seqlens_q / cu_seqlens_k: device int32 arrays of B + 1 entries.  Sequence b owns query tokens
 *             [cu_q[b], cu_q[b+1]) and key tokens [cu_k[b], cu_k[b+1]) and attends only to its own keys.  max_seqlen_q /
 *             max_seqlen_k (host) size the grid, as in flash-attn.  Tokens outside every sequence are not written.
 *   Causal.   Bottom-right aligned: query i of a sequence of N_q queries and N_k keys sees key j iff j <= i + (N_k - N_q);
 *             with N_q == N_k this is fa2_fwd's causal mask.
 *   Window.   window_left / window_right with the same shift: i + (N_k - N_q) - left <= j <= i + (N_k - N_q) + right,
 *             -1 = unbounded; causal clamps right to 0.  With N_q == N_k this is fa2_fwd_window's definition.
 *   Empty rows.  A row without a visible key (causal with N_q > N_k, N_k = 0, or a window) gets O = 0 and L = +inf, as
 *             FlashAttention-2 does: fa2_bwd_varlen then recomputes P = 0 for it, its dQ row is 0, no NaN anywhere.
 *   Lengths.  N_q = 0 and N_k = 0 are allowed.
 *   Dtypes.   f64, f32, f16, bf16; fp8 returns FA2_ERR_UNSUPPORTED (no backward, and e4m3fn cannot hold +inf).
 *   Safety.   Every cu_seqlens value read is clamped to [0, total]; end < start is empty; at most max_seqlen rows or keys of
 *             a sequence are processed.  Malformed offsets give wrong numbers at worst, never an access outside the tensors.
 *             Base pointers are built in 64 bits per sequence, so the 32-bit buffer-offset limit of the matrix kernels is
 *             judged on max_seqlen x row stride, not on the packed total.
 *
 * FA2_ERR_BAD_ARG before any launch for: a null pointer, B not in [1, 65535], H not in [1, 65535], max_seqlen_q / max_seqlen_k
 * not in [0, 2^28], total_q / total_k < 0, a window side < -1, a negative stride; the message names the argument.
 * Variants: FA2_VARIANT_AUTO (MFMA16D_W4 where it runs, else GENERIC), FA2_VARIANT_GENERIC (f64, f32, f16,
 * bf16, any strides, any d in [1, 512]), FA2_VARIANT_MFMA16D and FA2_VARIANT_MFMA16D_W4 (f16 / bf16, d in {64, 128}, unit
 * d-stride, 16-byte aligned rows).  Any other forced variant returns FA2_ERR_UNSUPPORTED.
 */
int fa2_fwd_varlen(const void *Q, const void *K, const void *V, void *O, void *L,
                   const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                   const int64_t o_strides[3], int64_t l_head_stride,
                   const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                   int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                   int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                   void *hip_stream);

int fa2_fwd_varlen_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                           const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                           const int64_t o_strides[3], int64_t l_head_stride,
                           const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                           int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                           int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                           int32_t window_right, void *hip_stream, int32_t variant);

/*
 * Grouped-query (GQA) and multi-query (MQA) attention: K and V have H_kv heads, 1 <= H_kv, H % H_kv == 0; with g = H / H_kv,
 * query head h attends with KV head h / g (the contiguous grouping of flash-attn and torch's enable_gqa).  Q, O, L keep H heads.
 *
 *   fa2_fwd_gqa(_variant): the arguments of fa2_fwd_window(_variant) with H_kv after H; K and V are (B, H_kv, N, d) with their own
 *   strides.  (window_left, window_right) = (-1, -1) is no window; windows are normalised as fa2_fwd_window normalises them.
 *   fa2_fwd_varlen_gqa(_variant): the arguments of fa2_fwd_varlen(_variant) with H_kv after H; K and V are (total_k, H_kv, d).
 *
 * FA2_ERR_BAD_ARG before any launch for H_kv < 1 or H % H_kv != 0 ("H_kv" in the message); every check of the non-GQA entry point
 * applies as well.  H_kv == H runs the non-GQA entry point itself (fa2_fwd_window(_variant), fa2_fwd_varlen(_variant)): the same
 * results bit for bit, the same variants.
 *
 * Dense layouts.  A layout is MERGEABLE when B == 1, or when the batch strides of Q, O and L are H times their head strides and
 * those of K and V H_kv times theirs (the contiguous (B, H, N, d) layout, a B = 1 (B, N, H, d) view); with H_kv = 1 the head
 * stride of K and V is not read, so any stride of that size-1 dimension merges.  Such a problem runs as the MHA
 * problem of B * H_kv batches of g heads that share one K / V head (head stride 0), on the kernels and the table of fa2_fwd /
 * fa2_fwd_window, so every variant they take is accepted (fp8 included) and AUTO picks what it picks for the same B * H.  Any other
 * layout runs GQA forms of the windowed kernels, a plain or causal problem as the full band: FA2_VARIANT_AUTO (MFMA16D / MFMA16D_W4
 * for f16 / bf16 at d 64 / 128, else GENERIC), FA2_VARIANT_GENERIC (every dtype, fp8 included), FA2_VARIANT_MFMA16D and
 * FA2_VARIANT_MFMA16D_W4.
 * Varlen.  FA2_VARIANT_AUTO (MFMA16D_W4 where it runs, else GENERIC), FA2_VARIANT_GENERIC, FA2_VARIANT_MFMA16D and
 * FA2_VARIANT_MFMA16D_W4, as fa2_fwd_varlen.  Any other forced variant returns FA2_ERR_UNSUPPORTED.
 */
int fa2_fwd_gqa(const void *Q, const void *K, const void *V, void *O, void *L,
                const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                const int64_t o_strides[4], const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv,
                int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                int32_t window_right, void *hip_stream);

int fa2_fwd_gqa_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                        const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                        const int64_t o_strides[4], const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv,
                        int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                        int32_t window_right, void *hip_stream, int32_t variant);

int fa2_fwd_varlen_gqa(const void *Q, const void *K, const void *V, void *O, void *L,
                       const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                       const int64_t o_strides[3], int64_t l_head_stride,
                       const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t H_kv,
                       int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                       int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                       void *hip_stream);

int fa2_fwd_varlen_gqa_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                               const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                               const int64_t o_strides[3], int64_t l_head_stride,
                               const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                               int32_t H_kv, int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                               int32_t total_k, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                               int32_t window_right, void *hip_stream, int32_t variant);

/*
 * Packed attention with a value head size of its own (un-absorbed MLA prefill: d = 192 = 128 "nope" + 64 rotary columns,
 * d_v = 128).  Forward only.
 *
 *   fa2_fwd_varlen_dv(_variant): the arguments of fa2_fwd_varlen_gqa(_variant) with d_v after d.  Q is (total_q, H, d), K is
 *   (total_k, H_kv, d), V is (total_k, H_kv, d_v), O is (total_q, H, d_v), L is (H, total_q); strides in elements, three per
 *   tensor.  d and d_v lie in [1, 512], H % H_kv == 0.  Offsets and their clamping, the bottom-right causal mask and window, empty
 *   rows (O = 0, L = +inf), zero-length sequences, tokens outside every sequence (not written), L's definition and dtype and the
 *   64-bit per-sequence base pointers are fa2_fwd_varlen's.  f64, f32, f16, bf16; fp8 returns FA2_ERR_UNSUPPORTED.
 *
 * Every error of fa2_fwd_varlen_gqa applies, from the same checks in the same order; then FA2_ERR_BAD_ARG ("d_v" in the message)
 * for d_v outside [1, 512], before any launch.
 * Variants of this entry point only: FA2_VARIANT_AUTO (MFMA16DV where it runs, else GENERIC; at d_v == d the table of
 * fa2_fwd_varlen_gqa), FA2_VARIANT_GENERIC (every dtype above, any strides, any d and d_v; at d_v == d the kernel and the bits of
 * fa2_fwd_varlen_gqa_variant(GENERIC)) and FA2_VARIANT_MFMA16DV (f16 / bf16, d == 192, d_v == 128, unit d-stride, 16-byte aligned
 * rows of Q, K, V and O, scale > 0, max_seqlen_k x row stride below 2 GiB).  A forced MFMA16DV on a problem it cannot take, and any
 * other forced variant, return FA2_ERR_UNSUPPORTED.
 */
#define FA2_VARIANT_MFMA16DV 28 /* fa2_fwd_varlen_dv only: f16/bf16, d = 192, d_v = 128; MFMA16D_W4's tile with a two-image K unit */

int fa2_fwd_varlen_dv(const void *Q, const void *K, const void *V, void *O, void *L,
                      const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                      const int64_t o_strides[3], int64_t l_head_stride,
                      const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t H_kv,
                      int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                      int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                      void *hip_stream);

int fa2_fwd_varlen_dv_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                              const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                              const int64_t o_strides[3], int64_t l_head_stride,
                              const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                              int32_t H_kv, int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k,
                              int32_t total_q, int32_t total_k, int32_t dtype_enum, int32_t causal, float scale,
                              int32_t window_left, int32_t window_right, void *hip_stream, int32_t variant);

/*
 * Decode attention over a padded KV cache, split-KV (flash-decoding).  Forward only.
 *
 *   Shapes.   Q, O are (B, H, N_q, d), L is (B, H, N_q); K, V are (B, H_kv, S_k, d): S_k is the cache CAPACITY.  All strides are
 *             element strides in that logical order, as fa2_fwd_gqa takes them (a flash-attn (B, S, H, d) cache is a transposed
 *             view); l_strides = {LB, LH}, unit stride over N_q.  H % H_kv == 0, query head h reads KV head h / (H / H_kv).
 *   Lengths.  cache_seqlens: device int32 array of B entries; sequence b has N_k(b) = clamp(cache_seqlens[b], 0, S_k) keys.  A null
 *             pointer means N_k = S_k for every b.  Rows >= N_k(b) of K and V are never read: they may hold anything, NaN included.
 *   Mask.     causal and (window_left, window_right) are fa2_fwd_varlen's definitions, bottom-right aligned with the shift
 *             N_k(b) - N_q; with N_q = 1 causal masks nothing.  A row without a visible key gets O = 0 and L = +inf.
 *   Dtypes.   f64, f32, f16, bf16; fp8 returns FA2_ERR_UNSUPPORTED, as in varlen (an fp8 CACHE under 16-bit Q: fa2_fwd_kvcache_fp8
 *             below).  L is the log2-domain log-sum-exp in dtype_enum.
 *   Splits.   The keys of a sequence are split across num_splits workgroups: split s covers keys [s c, (s + 1) c) with
 *             c = ceil(N_k(b) / num_splits) rounded up to 64.  num_splits = 0 picks fa2_kvcache_num_splits(...), a host heuristic
 *             on the capacity.  With num_splits > 1 the split kernels leave fp32 partials in `workspace` and a second launch on the
 *             same stream combines them; the caller owns the workspace (fa2_kvcache_workspace_bytes(...) bytes, 16-byte aligned,
 *             uninitialised is fine) and may reuse it once the stream has passed the call.  With num_splits resolving to 1 the
 *             workspace is neither read nor written and may be null.
 *   Variants. FA2_KVCACHE_VARIANT_MFMA16: f16 / bf16, d in {64, 128}, unit d-stride, 16-byte aligned rows, scale > 0 and
 *             (H / H_kv) * N_q <= 64: the query heads of a group share one matrix tile, so K and V are read once per KV head.
 *             FA2_KVCACHE_VARIANT_GENERIC: every dtype above, any strides, any d in [1, 512], any N_q, on the VALU; K and V are read
 *             once per query head and large N_q is correct but not a performance goal.  FA2_KVCACHE_VARIANT_AUTO: MFMA16 where it
 *             runs, else GENERIC.  A forced MFMA16 on a problem it cannot run returns FA2_ERR_UNSUPPORTED.
 *
 * FA2_ERR_BAD_ARG before any launch, the message naming the argument, for: null Q / K / V / O / L or strides, B or H outside
 * [1, 65535], H_kv < 1 or H % H_kv != 0 ("H_kv"), N_q < 1, S_k < 1, N_q or S_k > 2^28, B * H * N_q > 2^40, a window side < -1, a negative stride,
 * num_splits < 0 or > FA2_KVCACHE_MAX_SPLITS, num_splits resolving to more than 1 with a null or too small workspace ("workspace").
 * FA2_ERR_UNSUPPORTED for fp8, an unknown dtype or variant, d outside [1, 512].
 */
#define FA2_KVCACHE_VARIANT_AUTO 0
#define FA2_KVCACHE_VARIANT_GENERIC 1
#define FA2_KVCACHE_VARIANT_MFMA16 2
#define FA2_KVCACHE_MAX_SPLITS 128

int fa2_fwd_kvcache(const void *Q, const void *K, const void *V, void *O, void *L,
                    const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                    const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                    int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum,
                    int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                    void *workspace, int64_t workspace_bytes, void *hip_stream);

int fa2_fwd_kvcache_variant(const void *Q, const void *K, const void *V, void *O, void *L,
                            const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                            const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                            int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum,
                            int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                            void *workspace, int64_t workspace_bytes, void *hip_stream, int32_t variant);

/*
 * The same decode over an fp8 KV cache.  K and V hold OCP e4m3fn or e5m2 bytes (kv_dtype_enum: FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2,
 * the same for both) with one dequantisation scale per (sequence, KV head):
 *
 *     K = k_descale[b, h_kv] * float(K8),   V = v_descale[b, h_kv] * float(V8),
 *
 * and the result is fa2_fwd_kvcache's on those K and V: the same lengths, mask, split rule, workspace, variants and empty rows.  Q, O
 * and L stay f16 / bf16 (dtype_enum) and the matrix work stays 16-bit: fp8 -> f16 / bf16 is exact, so the kernels stage the converted
 * bytes, use scale * k_descale as the softmax scale of the workgroup and multiply the fp32 output by v_descale before it is rounded
 * (or written as a partial).  With both descales 1 the result equals fa2_fwd_kvcache's on the converted cache bit for bit.
 *
 *   Descales. k_descale / v_descale: device fp32, element [b, h_kv] at b * strides[0] + h_kv * strides[1] (element strides, 0
 *             broadcasts an axis); a null pointer means 1 (its strides may then be null).  The values live on the device and are not
 *             checked: they must be finite and > 0, or O and L are undefined (no access depends on them).
 *   Strides.  In elements of each tensor's own dtype: k_strides / v_strides count fp8 elements.
 *   Variants. FA2_KVCACHE_VARIANT_MFMA16 under fa2_fwd_kvcache's conditions, the 16-byte row alignment counted in fp8 bytes (K and V
 *             strides multiples of 16 elements); GENERIC takes everything else (any d in [1, 512], any strides, any N_q).
 *   Splits.   fa2_kvcache_workspace_bytes(...) and fa2_kvcache_num_splits(..., dtype_enum) as for fa2_fwd_kvcache.
 *
 * Every FA2_ERR_BAD_ARG of fa2_fwd_kvcache applies unchanged; also a negative descale stride and a non-null descale with null strides.
 * FA2_ERR_UNSUPPORTED, naming the argument, for a kv_dtype_enum that is not one of the two fp8 formats, a dtype_enum that is not
 * f16 / bf16, d outside [1, 512], an unknown variant, a forced MFMA16 on a problem it cannot run.
 */
int fa2_fwd_kvcache_fp8(const void *Q, const void *K, const void *V, void *O, void *L,
                        const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                        const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                        const float *k_descale, const float *v_descale,
                        const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                        int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d,
                        int32_t dtype_enum, int32_t kv_dtype_enum,
                        int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                        void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/*
 * The same decode over a PAGED KV cache: a pool of fixed-size pages and an int32 block table per sequence (vLLM, flash-attn's
 * flash_attn_with_kvcache(..., block_table=)).  Addressing only: lengths, mask, split rule, workspace, variants, empty rows, the fp8
 * formats and their descales are fa2_fwd_kvcache_fp8's, and on the cache a pool was scattered from the result is the contiguous
 * call's bit for bit.  kv_dtype_enum == dtype_enum with null descales is the 16-bit (f32, f64) pool.
 *
 *   Pool.     K, V are logically (num_blocks, H_kv, page_size, d); k_strides / v_strides are element strides in that order, index 0
 *             the BLOCK stride.  Any strides: a flash-attn (num_blocks, page_size, H_kv, d) pool is its transposed view.
 *   Table.    block_table: device int32, logically (B, max_blocks), entry [b, i] at b * block_table_stride + i.  Key j of sequence
 *             b, KV head hk, is the row at
 *                 pool + block_table[b, j / page_size] * strides[0] + hk * strides[1] + (j % page_size) * strides[2],
 *             formed in 64 bits.  Two sequences may name the same page.
 *   Capacity. max_blocks * page_size plays S_k's role everywhere: N_k(b) = clamp(cache_seqlens[b], 0, max_blocks * page_size), the
 *             split rule, and the S_k argument of fa2_kvcache_num_splits(...) that num_splits = 0 resolves to.
 *   Entries.  The table lives on the device and is not validated.  The kernels clamp every entry they read to
 *             [0, num_blocks - 1] before they form an address: a bad entry gives a wrong result for that sequence, never an access
 *             outside the pool.  Entries of pages at or beyond ceil(N_k(b) / page_size) do not influence the output; pool pages no
 *             visible key maps to, and the rows of a sequence's last page at or beyond N_k(b), are never read.
 *   Variants. FA2_KVCACHE_VARIANT_MFMA16 under fa2_fwd_kvcache_fp8's conditions (the block stride aligned like the others) and
 *             page_size % 64 == 0: a key tile then never straddles a page.  GENERIC takes any page_size >= 1 and everything else;
 *             AUTO picks MFMA16 where it runs.
 *
 * Every error of fa2_fwd_kvcache_fp8 applies, the capacity in S_k's place.  FA2_ERR_BAD_ARG also for a null block_table, num_blocks,
 * page_size or max_blocks < 1, max_blocks * page_size > 2^28, a negative block_table_stride, descales with kv_dtype_enum == dtype_enum.
 */
int fa2_fwd_kvcache_paged(const void *Q, const void *K, const void *V, void *O, void *L,
                          const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                          const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                          const int32_t *block_table, int64_t block_table_stride,
                          const float *k_descale, const float *v_descale,
                          const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                          int32_t B, int32_t H, int32_t H_kv, int32_t N_q,
                          int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                          int32_t dtype_enum, int32_t kv_dtype_enum,
                          int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                          void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/*
 * Decode over a cache whose VALUE head size differs from the key's, and whose value may be a view of the key: multi-head latent
 * attention (MLA, DeepSeek-V2 / V3 / R1, Kimi) in its absorbed form, where every query head of a token attends over ONE shared
 * latent row per key -- 512 latent columns followed by 64 rotary columns; the score takes all 576, the value is the first 512 of
 * the same row: H_kv = 1, d = 576, d_v = 512, V = K[..., :512].  Forward only.
 *
 *   Shapes.   Q is (B, H, N_q, d), K (B, H_kv, S_k, d), V (B, H_kv, S_k, d_v), O (B, H, N_q, d_v), L (B, H, N_q); d in [1, 576], d_v in
 *             [1, 512].  V may overlap K in memory: neither is written.  Everything else is fa2_fwd_kvcache's, unchanged: lengths
 *             and clamping, the bottom-right mask and window, empty rows (O = 0, L = +inf), the split rule, fp32 partials and the
 *             combine launch, L in the log2 domain.
 *   Cache.    block_table non-null: fa2_fwd_kvcache_paged's pool (num_blocks, H_kv, page_size, d) / (..., d_v), table and capacity
 *             max_blocks * page_size.  block_table null: the contiguous cache, a pool of one page per sequence -- page_size
 *             carries S_k, strides[0] is the batch stride, and num_blocks, max_blocks and block_table_stride are not read.
 *   Dtypes.   f16, bf16, f32, f64 (dtype_enum, the cache alike); an fp8 cache and its descales: fa2_fwd_kvcache_mla_fp8 below.
 *   Splits.   The workspace is fa2_kvcache_workspace_bytes(B, H, N_q, d_v, num_splits): the partials have d_v columns.
 *             num_splits = 0 resolves to fa2_kvcache_mla_num_splits(...).
 *   Variants. FA2_KVCACHE_VARIANT_MLA16 (this entry point only): f16 / bf16, d = 576 and d_v = 512, V aliasing K (the same base
 *             pointer, the same four strides), unit d-stride, 16-byte aligned rows (and workspace), scale > 0, any H_kv and any
 *             (H / H_kv) * N_q, contiguous or paged with page_size % 64 == 0.  One workgroup per 64 rows of a KV group stages each
 *             64-key tile of the latent cache once and reads the value operand from the same LDS image.
 *             FA2_KVCACHE_VARIANT_GENERIC: everything else (every dtype, any strides, any page size, a V that is a tensor of its
 *             own).  FA2_KVCACHE_VARIANT_AUTO: MLA16 where it runs, else GENERIC.  A forced MLA16 on a problem it cannot run
 *             returns FA2_ERR_UNSUPPORTED; FA2_KVCACHE_VARIANT_MFMA16 is not a variant of this call.
 *
 * Every FA2_ERR_BAD_ARG and FA2_ERR_UNSUPPORTED of fa2_fwd_kvcache_paged applies (with block_table null: S_k = page_size in the
 * capacity's place, no table errors), the message naming the argument; FA2_ERR_UNSUPPORTED also for d outside [1, 576] and d_v outside
 * [1, 512].  Not covered (use the d_v == d entry points): the append calls and rotary, packed queries.
 */
#define FA2_KVCACHE_VARIANT_MLA16 3

int fa2_fwd_kvcache_mla(const void *Q, const void *K, const void *V, void *O, void *L,
                        const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                        const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                        const int32_t *block_table, int64_t block_table_stride,
                        int32_t B, int32_t H, int32_t H_kv, int32_t N_q,
                        int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                        int32_t dtype_enum,
                        int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                        void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/* What num_splits = 0 resolves to for fa2_fwd_kvcache_mla, in [1, FA2_KVCACHE_MAX_SPLITS]: for f16 / bf16 at d = 576, d_v = 512 (the
 * matrix form, one workgroup per CU) the unsplit launch has B * H_kv * ceil((H / H_kv) * N_q / 64) workgroups; 1 when that is 256
 * or more, else enough splits for one workgroup per CU, every split at least 4 key tiles (256 keys) of the capacity S_k.  Any
 * other shape is counted as fa2_kvcache_num_splits counts the VALU form. */
int32_t fa2_kvcache_mla_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t d_v,
                                   int32_t dtype_enum);

/*
 * fa2_fwd_kvcache_mla over an fp8 latent cache: only the STORAGE is fp8, exactly as in fa2_fwd_kvcache_fp8.  K and V are OCP e4m3fn or
 * e5m2 bytes (kv_dtype_enum FA2_DTYPE_F8E4M3 / FA2_DTYPE_F8E5M2) under f16 / bf16 Q, O and L (dtype_enum), converted exactly to the
 * I/O dtype while they are staged; the matrix work stays 16-bit.  K = k_descale * float(K8), V = v_descale * float(V8), the descales
 * as in fa2_fwd_kvcache_paged: fp32 on the device at [b * strides[0] + h_kv * strides[1]], null = 1, finite and > 0; k_descale is
 * folded into the softmax scale, v_descale into the fp32 output.  With V a view of K (the latent cache) the two are still
 * independent scalars; a cache quantised as one tensor passes the same descale twice.  Strides of K and V are in elements of the
 * cache dtype (bytes).
 *
 *   kv_dtype_enum == dtype_enum with null descales is fa2_fwd_kvcache_mla: the same checks, the same launches.
 *   Splits and workspace do not depend on the cache dtype: fa2_kvcache_mla_num_splits, fa2_kvcache_workspace_bytes(B, H, N_q, d_v, n).
 *   Variants. FA2_KVCACHE_VARIANT_MLA16 over an fp8 cache: fa2_fwd_kvcache_mla's rule with the row starts 16-byte aligned in BYTES --
 *             every stride of K a multiple of 16 elements, the base 16-byte aligned -- V aliasing K, unit d-stride, page_size % 64 == 0
 *             when paged.  FA2_KVCACHE_VARIANT_GENERIC: every d <= 576 and d_v <= 512, any strides, any page size, a V tensor of its
 *             own.  FA2_KVCACHE_VARIANT_AUTO: MLA16 where it runs, else GENERIC.
 *
 * Errors: fa2_fwd_kvcache_mla's, and fa2_fwd_kvcache_paged's for the cache dtype and the descales -- a kv_dtype_enum that is neither
 * dtype_enum nor an fp8 format and f32 / f64 Q under an fp8 cache FA2_ERR_UNSUPPORTED, descales with a 16-bit cache and negative
 * descale strides FA2_ERR_BAD_ARG.
 */
int fa2_fwd_kvcache_mla_fp8(const void *Q, const void *K, const void *V, void *O, void *L,
                            const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                            const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                            const int32_t *block_table, int64_t block_table_stride,
                            const float *k_descale, const float *v_descale,
                            const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                            int32_t B, int32_t H, int32_t H_kv, int32_t N_q,
                            int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                            int32_t dtype_enum, int32_t kv_dtype_enum,
                            int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                            void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/*
 * Variable-length (packed) queries over the KV cache: every sequence brings its own number of query tokens -- a chunk of a prompt
 * over its cached prefix (chunked prefill, prefix caching), the draft tokens of speculative decoding, one decode token -- in one
 * call (flash-attn's flash_attn_varlen_func(..., block_table=)).  Forward only.  The keys of a chunk's own tokens are already in
 * the cache: the caller has appended them (fa2_kvcache_append).
 *
 *   Queries.  Q, O are packed (total_q, H, d), strides {token, head, dim} in elements (3 each); L is (H, total_q) in the I/O dtype,
 *             unit stride over tokens, head stride l_head_stride: fa2_fwd_varlen's layout.  cu_seqlens_q: device int32, B + 1
 *             entries; sequence b owns the n_q(b) = clamp(cu[b + 1] - cu[b], 0, max_seqlen_q) rows from clamp(cu[b], 0, total_q)
 *             on, every value read clamped to [0, total_q] as in fa2_fwd_varlen.  n_q(b) = 0 is legal.  Rows outside every
 *             sequence -- gaps between sequences, the rows of a sequence past max_seqlen_q -- are neither read nor written.
 *   Cache.    fa2_fwd_kvcache_paged's: with block_table the pool (num_blocks, H_kv, page_size, d) and its table, S_k ignored, the
 *             capacity max_blocks * page_size; with a null block_table the contiguous cache (B, H_kv, S_k, d) of capacity S_k,
 *             num_blocks / page_size / max_blocks ignored.  kv_dtype_enum == dtype_enum with null descales is the cache in Q's
 *             dtype, an fp8 kv_dtype_enum the fp8 cache of fa2_fwd_kvcache_fp8.  N_k(b) = clamp(cache_seqlens[b], 0, capacity), a
 *             null cache_seqlens the capacity.  Rows at or beyond N_k(b), pool pages no visible key maps to and table entries past
 *             a sequence's pages are never read; table entries are clamped into the pool before an address is formed.
 *   Mask.     fa2_fwd_varlen's band of n_q(b) queries and N_k(b) keys, bottom-right aligned per sequence: query i of sequence b
 *             stands at position N_k(b) - n_q(b) + i.  A row without a visible key (N_k(b) < n_q(b) under causal, N_k(b) = 0, a
 *             window) gets O = 0 and L = +inf.
 *   Splits.   fa2_fwd_kvcache's rule on each sequence's own length, every (query tile, KV head, sequence) split alike;
 *             num_splits = 0 picks fa2_kvcache_varlen_num_splits(...).  Workspace: fa2_kvcache_varlen_workspace_bytes(...) bytes,
 *             16-byte aligned, uninitialised is fine; untouched (and may be null) when num_splits resolves to 1.
 *   Variants. FA2_KVCACHE_VARIANT_MFMA16: f16 / bf16, d in {64, 128}, g = H / H_kv <= 64, unit d-stride, 16-byte aligned rows,
 *             scale > 0, page_size % 64 == 0 when paged.  A workgroup owns tq = min(64 / g, max_seqlen_q) consecutive query
 *             positions of one sequence for the g heads of a KV group, so K and V are read once per (KV head, query tile).  With
 *             every n_q(b) = max_seqlen_q = N_q and g * N_q <= 64 the tile is fa2_fwd_kvcache's and, at the same explicit
 *             num_splits, O and L equal that call's bit for bit.  FA2_KVCACHE_VARIANT_GENERIC: everything else, 16 query rows per
 *             workgroup on the VALU.  AUTO: MFMA16 where it runs.  A forced MFMA16 it cannot run returns FA2_ERR_UNSUPPORTED.
 *
 * Every error of fa2_fwd_kvcache_paged applies (S_k in the capacity's place for a contiguous cache, max_seqlen_q in N_q's).
 * FA2_ERR_BAD_ARG also for a null cu_seqlens_q, total_q < 1, max_seqlen_q < 1 or > 2^28, total_q * H > 2^40, a negative
 * l_head_stride; the message names the argument.
 */
int fa2_fwd_kvcache_varlen(const void *Q, const void *K, const void *V, void *O, void *L,
                           const int64_t q_strides[3], const int64_t k_strides[4], const int64_t v_strides[4],
                           const int64_t o_strides[3], int64_t l_head_stride,
                           const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                           const int32_t *block_table, int64_t block_table_stride,
                           const float *k_descale, const float *v_descale,
                           const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                           int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                           int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                           int32_t dtype_enum, int32_t kv_dtype_enum,
                           int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                           void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/* Bytes of workspace such a call needs: 0 for num_splits <= 1, else fp32 partial O [num_splits][total_q * H][d] followed by fp32
 * partial L [num_splits][total_q * H]. */
int64_t fa2_kvcache_varlen_workspace_bytes(int32_t total_q, int32_t H, int32_t d, int32_t num_splits);

/* What num_splits = 0 resolves to for it: fa2_kvcache_num_splits' rule with the unsplit workgroup count of the packed launch,
 * H_kv * min(B * ceil(max_seqlen_q / tq), ceil(total_q / tq) + B) for the matrix form (H and tq = 16 for the VALU form). */
int32_t fa2_kvcache_varlen_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                                      int32_t d, int32_t dtype_enum);

/*
 * The write side of a decode step: puts N_new new tokens of K and V into the cache, applies rotary embedding, and writes the new
 * lengths -- one launch (flash-attn's flash_attn_with_kvcache(..., k=, v=, rotary_cos=, rotary_sin=), without the attention).
 *
 *   Cache.    K, V with k_strides / v_strides are fa2_fwd_kvcache's cache (B, H_kv, S_k, d) when block_table is null (S_k is then the
 *             capacity and num_blocks, page_size, max_blocks are ignored), else fa2_fwd_kvcache_paged's pool, table and capacity
 *             max_blocks * page_size (S_k is then ignored).  They are written in place.  kv_dtype_enum is the cache's element type:
 *             dtype_enum, or an fp8 format under f16 / bf16 inputs.
 *   Tokens.   k_new, v_new: (B, H_kv, N_new, d) in dtype_enum, element strides in that order, any strides (a flash-attn
 *             (B, N_new, H_kv, d) tensor is its transposed view).  With start(b) = clamp(cache_seqlens[b], 0, capacity), token t of
 *             sequence b becomes key j = start(b) + t, addressed as the decode calls address key j (paged: row j % page_size of page
 *             block_table[b, j / page_size], the entry clamped to [0, num_blocks - 1], so a wild entry is a write to a wrong page of
 *             the pool and never one outside it; addresses in 64 bits).  Tokens with j >= capacity are dropped.  A run of tokens may
 *             straddle pages.  Two sequences that append into the same row of a shared page leave either one's bytes there: copy on
 *             write is the caller's, nothing detects it.
 *   Lengths.  cache_seqlens: device int32, B entries, read only.  seqlens_out: device int32, B entries, another buffer:
 *             seqlens_out[b] = min(start(b) + N_new, capacity) -- the cache_seqlens of the attention that follows and of the next step.
 *   Rotary.   rotary_cos, rotary_sin: device (S_rot, rotary_dim / 2) in dtype_enum, unit stride in the last axis, row strides
 *             rotary_cos_stride / rotary_sin_stride; both null: none.  rotary_dim is even, in [2, d]; columns >= rotary_dim pass
 *             through.  rotary_interleaved = 0 pairs column i with i + rotary_dim / 2 (GPT-NeoX), 1 pairs 2i with 2i + 1 (GPT-J).  K
 *             token t is rotated at position start(b) + t; V never.  Positions are clamped to S_rot - 1 before a table is read.
 *             (x1, x2) -> (x1 c - x2 s, x2 c + x1 s) in fp32 (f64 for f64), every product, sum and difference rounded on its own (no
 *             FMA), then one rounding to nearest even to the cache's dtype.
 *   Q.        Optional: Q (B, H, N_q, d) with q_strides, rotated into the caller's contiguous q_rot (B, H, N_q, d) in dtype_enum; Q is
 *             not modified.  Row i is rotated at start(b) + i when q_pos_per_row is non-zero (what a causal or windowed attention
 *             wants), every row at start(b) otherwise.  Without tables Q and q_rot are not touched.  A null Q (H, N_q, q_strides are
 *             then ignored) updates the cache alone: what a prefill uses to fill it.
 *   fp8.      The stored byte is fp8(clamp(x / descale[b, h_kv], +-max)), max = 448 (e4m3fn) / 57344 (e5m2): x the fp32 value (after
 *             rotary for K, not rounded to 16 bits in between), a correctly rounded fp32 division, conversion to nearest even -- the
 *             rule of a cache quantised with these descales.  Descales as in fa2_fwd_kvcache_fp8; null means 1.
 *
 * FA2_ERR_BAD_ARG before any launch, the message naming the argument: null K / V / k_new / v_new / their strides / cache_seqlens /
 * seqlens_out; seqlens_out == cache_seqlens; N_new < 1 or > 2^28; B or H_kv outside [1, 65535]; S_k (contiguous) outside [1, 2^28];
 * with a table num_blocks, page_size or max_blocks < 1, max_blocks * page_size > 2^28, a negative block_table_stride; a negative
 * stride; descales with kv_dtype_enum == dtype_enum, a descale with null or negative strides; exactly one of rotary_cos / rotary_sin;
 * rotary_dim odd, < 2 or > d; S_rot < 1; tables and Q with a null q_rot; with Q, null q_strides, H outside [1, 65535], H % H_kv != 0
 * ("H_kv"), N_q outside [1, 2^28].  FA2_ERR_UNSUPPORTED for a kv_dtype_enum that is neither dtype_enum nor an fp8 format, an fp8 cache
 * under inputs that are not f16 / bf16, fp8 or unknown dtype_enum, d outside [1, 512].
 */
int fa2_kvcache_append(void *K, void *V, const int64_t k_strides[4], const int64_t v_strides[4],
                       const int32_t *block_table, int64_t block_table_stride,
                       const void *k_new, const void *v_new, const int64_t k_new_strides[4], const int64_t v_new_strides[4],
                       const int32_t *cache_seqlens, int32_t *seqlens_out,
                       const float *k_descale, const float *v_descale,
                       const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                       const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                       int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                       const void *Q, void *q_rot, const int64_t q_strides[4], int32_t H, int32_t N_q, int32_t q_pos_per_row,
                       int32_t B, int32_t H_kv, int32_t N_new, int32_t S_k,
                       int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                       int32_t dtype_enum, int32_t kv_dtype_enum, void *hip_stream);

/*
 * The fused decode step: fa2_kvcache_append, then on the same stream the decode attention over the updated cache -- the contiguous
 * (block_table null), fp8 (kv_dtype_enum != dtype_enum) or paged call, whichever the arguments select -- with seqlens_out as its
 * lengths, N_k(b) = seqlens_out[b], and, when the tables are given, q_rot in Q's place.  q_pos_per_row is
 * causal || window_left >= 0 || window_right >= 0.  Mask, split rule, num_splits, workspace, variants and empty rows are the existing
 * calls'; so is the guarantee that rows at or beyond N_k(b) never reach the output.  cache_seqlens is not modified.  q_rot may be
 * null without tables.  Every error of fa2_kvcache_append and of the selected decode call comes back before any launch.
 */
int fa2_fwd_kvcache_append(const void *Q, void *K, void *V, void *O, void *L,
                           const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                           const int64_t o_strides[4], const int64_t l_strides[2],
                           const int32_t *cache_seqlens, int32_t *seqlens_out,
                           const int32_t *block_table, int64_t block_table_stride,
                           const float *k_descale, const float *v_descale,
                           const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                           const void *k_new, const void *v_new, const int64_t k_new_strides[4], const int64_t v_new_strides[4],
                           const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                           int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, void *q_rot,
                           int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t N_new, int32_t S_k,
                           int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                           int32_t dtype_enum, int32_t kv_dtype_enum,
                           int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                           void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/*
 * The packed (ragged) form of fa2_kvcache_append: every sequence brings its own number of new tokens -- a chunk of a prompt beside
 * one-token decodes -- in one launch.  Cache, lengths, rotary arithmetic, fp8 rule, paging and every guarantee are fa2_kvcache_append's;
 * what differs:
 *
 *   Tokens.   k_new, v_new: packed (total_new, H_kv, d) in dtype_enum, strides {token, head, dim} in elements (3 each), any
 *             non-negative strides.  cu_seqlens_new: device int32, B + 1 entries.  Sequence b brings n_new(b) =
 *             clamp(cu[b + 1] - cu[b], 0, max_seqlen_new) rows from s(b) = cu[b] on, every offset read clamped to [0, total_new] as
 *             in fa2_fwd_kvcache_varlen; n_new(b) = 0 is legal.  Row s(b) + t becomes key j = start(b) + t of sequence b and K is
 *             rotated at min(j, S_rot - 1); tokens with j >= capacity are dropped.  Rows outside every sequence -- in front of the
 *             first offset, the surplus of a span longer than max_seqlen_new, behind the last offset -- are not read.
 *   Lengths.  seqlens_out[b] = min(start(b) + n_new(b), capacity), written for every b, sequences without tokens included.
 *   Q.        Optional, with tables: Q packed (total_new, H, d) over the same cu_seqlens_new, q_strides {token, head, dim}, rotated
 *             into the caller's contiguous packed q_rot (total_new, H, d).  Row i of sequence b is rotated at
 *             min(start(b) + (q_pos_per_row ? i : 0), S_rot - 1).  Rows of q_rot outside every sequence are not written.
 *   Work.     One thread row per packed row (a binary search over cu_seqlens_new finds its sequence), not B x max_seqlen_new
 *             tiles: a long chunk beside many one-token decodes costs what its total_new rows cost.
 *   Offsets.  For non-decreasing cu_seqlens_new the result is exactly the per-sequence definition above.  For offsets that are not
 *             non-decreasing the cache may receive wrong rows; every address formed is still inside k_new / v_new / Q / q_rot (row
 *             < total_new), the cache or pool (key index < capacity, page clamped), the block table (b < B, page slot < max_blocks)
 *             and the rotary tables: wrong numbers at worst, never an access outside the tensors.
 *
 * Every error of fa2_kvcache_append applies (N_new and N_q do not exist here).  FA2_ERR_BAD_ARG also for a null cu_seqlens_new,
 * total_new or max_seqlen_new outside [1, 2^28], total_new * max(H, 2 * H_kv) > 2^40 (H counted only with Q; the bound of B * H * N_q in
 * the decode calls, which keeps every byte offset of a row far inside 64 bits); the message names the argument.
 */
int fa2_kvcache_append_varlen(void *K, void *V, const int64_t k_strides[4], const int64_t v_strides[4],
                              const int32_t *block_table, int64_t block_table_stride,
                              const void *k_new, const void *v_new, const int64_t k_new_strides[3], const int64_t v_new_strides[3],
                              const int32_t *cu_seqlens_new, const int32_t *cache_seqlens, int32_t *seqlens_out,
                              const float *k_descale, const float *v_descale,
                              const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                              const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                              int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                              const void *Q, void *q_rot, const int64_t q_strides[3], int32_t H, int32_t q_pos_per_row,
                              int32_t B, int32_t H_kv, int32_t total_new, int32_t max_seqlen_new, int32_t S_k,
                              int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                              int32_t dtype_enum, int32_t kv_dtype_enum, void *hip_stream);

/*
 * The fused ragged step (a mixed batch of chunked prefill and decodes in one call): fa2_kvcache_append_varlen, then on the same stream
 * fa2_fwd_kvcache_varlen over the updated cache with seqlens_out as its cache_seqlens and cu_seqlens_q as the append's
 * cu_seqlens_new -- total_new = total_q, max_seqlen_new = max_seqlen_q, and token i of Q, k_new and v_new is the same token.  With
 * tables the attention reads q_rot (packed, contiguous) in Q's place; q_rot may be null without them.  q_pos_per_row is
 * causal || window_left >= 0 || window_right >= 0, fa2_fwd_kvcache_append's rule, so a uniform batch reproduces that call.
 * cache_seqlens holds the lengths BEFORE the append and is not modified.  Mask, split rule, num_splits, workspace, variants and
 * empty rows are fa2_fwd_kvcache_varlen's.  Every error of both halves comes back before any launch.
 */
int fa2_fwd_kvcache_varlen_append(const void *Q, void *K, void *V, void *O, void *L,
                                  const int64_t q_strides[3], const int64_t k_strides[4], const int64_t v_strides[4],
                                  const int64_t o_strides[3], int64_t l_head_stride,
                                  const int32_t *cu_seqlens_q, const int32_t *cache_seqlens, int32_t *seqlens_out,
                                  const int32_t *block_table, int64_t block_table_stride,
                                  const float *k_descale, const float *v_descale,
                                  const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                                  const void *k_new, const void *v_new, const int64_t k_new_strides[3], const int64_t v_new_strides[3],
                                  const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                                  int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, void *q_rot,
                                  int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                                  int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d,
                                  int32_t dtype_enum, int32_t kv_dtype_enum,
                                  int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                                  void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/*
 * The write side of the latent (MLA) cache of fa2_fwd_kvcache_mla / _mla_fp8: fa2_kvcache_append for a cache that is ONE tensor
 * whose rows hold d_v latent columns followed by d - d_v positional ones.  Lengths, clamps, the drop of tokens past the capacity,
 * paging, the rotary arithmetic and the fp8 rule are fa2_kvcache_append's; what differs:
 *
 *   Cache.    KV: (B, H_kv, S_k, d) or, with block_table, the pool (num_blocks, H_kv, page_size, d), strides kv_strides, in
 *             kv_dtype_enum (dtype_enum, or an fp8 format under f16 / bf16 inputs).  It is written once: the value of the decode
 *             call is a view of the same rows.  d in [2, 576], d_v in [1, d - 1].
 *   Sources.  A new row comes from two tensors in dtype_enum, each with strides of its own: c_new (B, H_kv, N_new, d_v) fills
 *             columns [0, d_v), pe_new (B, H_kv, N_new, d - d_v) columns [d_v, d).  One (B, H_kv, N_new, d) tensor X is the call
 *             with c_new = X, pe_new = X + d_v * (its d-stride) and both stride arrays X's.
 *   Rotary.   With tables, columns [d_v, d_v + rotary_dim) -- pe_new's first rotary_dim -- are rotated at min(j, S_rot - 1) for
 *             key index j; the pairing (i with i + rotary_dim / 2, or 2i with 2i + 1 when rotary_interleaved) is applied inside
 *             that range, table column i belongs to pair i of it.  Columns before and behind the range are copied (16-bit / f32 /
 *             f64 cache: bit for bit).  rotary_dim even, in [2, d - d_v].
 *   fp8.      One descale for the whole row: kv_descale at [b * s[0] + h_kv * s[1]], null = 1, the stored byte
 *             fp8(clamp(x / kv_descale)) of the unrounded fp32 value, as in fa2_kvcache_append.
 *   Q.        Optional, with tables: Q (B, H, N_q, d), any strides, goes to the contiguous q_rot with the same columns
 *             [d_v, d_v + rotary_dim) rotated at fa2_kvcache_append's positions (q_pos_per_row); every other column is copied
 *             bit for bit.
 *   Speed.    16-byte loads and 16- or 8-byte stores when dtype_enum is f16 / bf16, every d-stride is 1, the other strides are
 *             multiples of 8, c_new, pe_new (and Q, q_rot, the tables) are 16-byte aligned, KV to 16 bytes (8 for an fp8 cache),
 *             d_v % 8 == 0, d % 8 == 0 and rotary_dim % 16 == 0; one element at a time otherwise, with the same bytes.
 *
 * Errors as fa2_kvcache_append's, before any launch, the message naming the argument (KV, kv_strides, c_new, pe_new,
 * c_new_strides, pe_new_strides, kv_descale, kv_descale_strides in K / V's places); FA2_ERR_UNSUPPORTED for d outside [2, 576] or
 * d_v outside [1, d - 1], FA2_ERR_BAD_ARG for a rotary_dim that is odd or outside [2, d - d_v].
 */
int fa2_kvcache_mla_append(void *KV, const int64_t kv_strides[4], const int32_t *block_table, int64_t block_table_stride,
                           const void *c_new, const void *pe_new, const int64_t c_new_strides[4], const int64_t pe_new_strides[4],
                           const int32_t *cache_seqlens, int32_t *seqlens_out,
                           const float *kv_descale, const int64_t kv_descale_strides[2],
                           const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                           int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                           const void *Q, void *q_rot, const int64_t q_strides[4], int32_t H, int32_t N_q, int32_t q_pos_per_row,
                           int32_t B, int32_t H_kv, int32_t N_new, int32_t S_k,
                           int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                           int32_t dtype_enum, int32_t kv_dtype_enum, void *hip_stream);

/*
 * The packed (ragged) form of fa2_kvcache_mla_append, as fa2_kvcache_append_varlen is fa2_kvcache_append's: c_new
 * (total_new, H_kv, d_v) and pe_new (total_new, H_kv, d - d_v) packed over cu_seqlens_new with strides {token, head, dim} (3
 * each), Q and q_rot packed (total_new, H, d).  Spans, empty sequences, gaps, max_seqlen_new, the lengths and every guarantee
 * about offsets are fa2_kvcache_append_varlen's, and so are its errors.
 */
int fa2_kvcache_mla_append_varlen(void *KV, const int64_t kv_strides[4], const int32_t *block_table, int64_t block_table_stride,
                                  const void *c_new, const void *pe_new, const int64_t c_new_strides[3], const int64_t pe_new_strides[3],
                                  const int32_t *cu_seqlens_new, const int32_t *cache_seqlens, int32_t *seqlens_out,
                                  const float *kv_descale, const int64_t kv_descale_strides[2],
                                  const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                                  int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                                  const void *Q, void *q_rot, const int64_t q_strides[3], int32_t H, int32_t q_pos_per_row,
                                  int32_t B, int32_t H_kv, int32_t total_new, int32_t max_seqlen_new, int32_t S_k,
                                  int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                                  int32_t dtype_enum, int32_t kv_dtype_enum, void *hip_stream);

/*
 * The fused MLA decode step: fa2_kvcache_mla_append, then on the same stream fa2_fwd_kvcache_mla (kv_dtype_enum == dtype_enum) or
 * fa2_fwd_kvcache_mla_fp8 over the updated cache with K = V = KV, v_strides = kv_strides, kv_descale for both descales, seqlens_out as
 * its cache_seqlens and, with tables, q_rot (contiguous (B, H, N_q, d)) as its Q; q_rot may be null without them.  q_pos_per_row
 * is causal || window_left >= 0 || window_right >= 0.  S_k is the capacity of a contiguous cache (block_table null), unlike
 * fa2_fwd_kvcache_mla, which passes it in page_size.  cache_seqlens holds the lengths BEFORE the append and is not modified.
 * num_splits and the workspace are fa2_kvcache_mla_num_splits' and fa2_kvcache_workspace_bytes(B, H, N_q, d_v, num_splits); the
 * variants are fa2_fwd_kvcache_mla's.  Every error of both halves comes back before any launch, and a forced
 * FA2_KVCACHE_VARIANT_MLA16 that cannot run the problem fails before the cache is written.
 */
int fa2_fwd_kvcache_mla_append(const void *Q, void *KV, void *O, void *L,
                               const int64_t q_strides[4], const int64_t kv_strides[4], const int64_t o_strides[4],
                               const int64_t l_strides[2], const int32_t *cache_seqlens, int32_t *seqlens_out,
                               const int32_t *block_table, int64_t block_table_stride,
                               const float *kv_descale, const int64_t kv_descale_strides[2],
                               const void *c_new, const void *pe_new, const int64_t c_new_strides[4], const int64_t pe_new_strides[4],
                               const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride, int64_t rotary_sin_stride,
                               int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved, void *q_rot,
                               int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t N_new, int32_t S_k,
                               int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                               int32_t dtype_enum, int32_t kv_dtype_enum,
                               int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                               void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/*
 * Variable-length (packed) queries over the latent cache: fa2_fwd_kvcache_varlen's queries on fa2_fwd_kvcache_mla's cache -- the
 * verification of MTP / draft tokens, a prefill chunk beside one-token decodes, a prefix-cached chunk, in one call.  Forward only.
 *
 *   Queries.  fa2_fwd_kvcache_varlen's: Q packed (total_q, H, d), O packed (total_q, H, d_v), strides {token, head, dim}; L
 *             (H, total_q) with head stride l_head_stride; cu_seqlens_q, max_seqlen_q, n_q(b) and the untouched rows as there.
 *   Cache.    KV with kv_strides is the one tensor of the latent cache: (B, H_kv, S_k, d) with a null block_table (num_blocks,
 *             page_size, max_blocks ignored), else the pool (num_blocks, H_kv, page_size, d) behind the table (S_k ignored).  The call
 *             is the attention with K = V = KV and v_strides = kv_strides: the score takes all d columns, the value the first d_v
 *             of the same row.  d in [1, 576], d_v in [1, 512].  kv_dtype_enum == dtype_enum with a null kv_descale is the cache
 *             in Q's dtype; an fp8 kv_dtype_enum the fp8 cache of fa2_fwd_kvcache_mla_fp8 with kv_descale (at [b *
 *             kv_descale_strides[0] + h_kv * kv_descale_strides[1]], null = 1) as K's and V's descale.  A V tensor of its own is
 *             not supported with packed queries.
 *   Mask.     fa2_fwd_kvcache_varlen's.
 *   Splits.   num_splits = 0 picks fa2_kvcache_mla_varlen_num_splits(...).  Workspace: fa2_kvcache_varlen_workspace_bytes(total_q,
 *             H, d_v, num_splits) bytes, 16-byte aligned.
 *   Variants. fa2_fwd_kvcache_mla's.  FA2_KVCACHE_VARIANT_MLA16: f16 / bf16, d = 576, d_v = 512, the cache in that dtype, e4m3 or
 *             e5m2, unit d-stride, 16-byte aligned rows (an fp8 cache: every stride a multiple of 16 elements), scale > 0,
 *             page_size % 64 == 0 when paged; any H_kv, any g = H / H_kv.  The g n_q(b) rows of a (sequence, KV head) are taken
 *             position-major, row = position * g + head, 64 to a workgroup, so the cache is read once per 64 rows whatever g.
 *             With every n_q(b) = max_seqlen_q = N_q O and L equal fa2_fwd_kvcache_mla's (_mla_fp8's) at the same explicit
 *             num_splits bit for bit.  GENERIC: everything else.  AUTO: MLA16 where it runs.
 *
 * Every error of fa2_fwd_kvcache_varlen and of fa2_fwd_kvcache_mla applies, with their messages.
 */
int fa2_fwd_kvcache_mla_varlen(const void *Q, const void *KV, void *O, void *L,
                               const int64_t q_strides[3], const int64_t kv_strides[4], const int64_t o_strides[3],
                               int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                               const int32_t *block_table, int64_t block_table_stride,
                               const float *kv_descale, const int64_t kv_descale_strides[2],
                               int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                               int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                               int32_t dtype_enum, int32_t kv_dtype_enum,
                               int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                               void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/* What num_splits = 0 resolves to for it: fa2_kvcache_mla_num_splits' rule (enough splits for one workgroup per CU) on the unsplit
 * workgroup count of the query-tiled latent form, H_kv * min(B * ceil(g * max_seqlen_q / 64), ceil(g * total_q / 64) + B) with
 * g = H / H_kv, every split at least 8 key tiles (512 keys) of the capacity, for f16 / bf16 at d 576 / d_v 512; every other shape as
 * fa2_kvcache_varlen_num_splits counts the VALU form. */
int32_t fa2_kvcache_mla_varlen_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                                          int32_t d, int32_t d_v, int32_t dtype_enum);

/*
 * Sparse MLA decode: every (sequence, KV head, query position) brings a list of key indices and attends over exactly those keys of
 * the latent cache (DeepSeek-V3.2's sparse attention, decode and sparse prefill chunks alike: an indexer picks the keys, this call is
 * the attention).  No row of the cache is gathered: each listed row is read where it lies.  Forward only.
 *
 *   Tensors.  fa2_fwd_kvcache_mla_fp8's: Q (B, H, N_q, d), the latent cache K (B, H_kv, S_k, d) or, with block_table, the pool
 *             (num_blocks, H_kv, page_size, d), V the first d_v columns of the same rows (or a tensor of its own: GENERIC), O
 *             (B, H, N_q, d_v), L (B, H, N_q) in the log2 domain; d in [1, 576], d_v in [1, 512], H_kv dividing H.  block_table null:
 *             the contiguous cache, page_size carries S_k, as in fa2_fwd_kvcache_mla.
 *   Indices.  int32 on the device, (B, H_kv, N_q, topk) with four element strides (index_strides, each >= 0, 0 allowed: one list
 *             for every KV head, say); topk >= 1.  Entry [b, hk, qi, s] is a logical key position j of sequence b -- through a
 *             block table row j % page_size of page block_table[b, j / page_size], the entry clamped into the pool, ANY page size.
 *             An entry with j < 0 or j >= N_k(b) (the clamp of cache_seqlens[b]; null: S_k) is no key: it is never turned into an
 *             address and its score is selected to -inf -- a shorter list is padded with -1.  A key listed twice counts twice.  A
 *             row without a valid entry gives O = 0 and L = +inf.
 *   Mask.     None: the list is the mask (the indexer respects causality).
 *   Splits.   Over the SLOTS of the list: split s covers slots [s c, (s + 1) c), c = ceil(topk / num_splits) rounded up to 64.
 *             Partials, workspace (fa2_kvcache_workspace_bytes(B, H, N_q, d_v, num_splits)) and the combine launch are
 *             fa2_fwd_kvcache_mla's.  num_splits = 0 resolves to fa2_kvcache_mla_sparse_num_splits(...).
 *   fp8.      As fa2_fwd_kvcache_mla_fp8: storage only, descales at [b, h_kv], folded into the softmax scale and the fp32 output;
 *             kv_dtype_enum == dtype_enum with null descales is the 16-bit (or f32 / f64) cache.  Unlike there a null descale is
 *             not read as 1: an fp8 cache brings both (a quantised cache has one; pass it twice), else FA2_ERR_BAD_ARG.
 *   Variants. FA2_KVCACHE_VARIANT_MLA16: f16 / bf16, the cache alike or fp8, d = 576 and d_v = 512, V aliasing K, the alignment
 *             rules of fa2_fwd_kvcache_mla(_fp8), any H_kv and H / H_kv, contiguous or paged with any page size: a workgroup owns 64
 *             heads of one (sequence, KV head, query position).  FA2_KVCACHE_VARIANT_GENERIC: everything else.  AUTO: MLA16 where
 *             it runs, else GENERIC.  A forced MLA16 on a problem it cannot run returns FA2_ERR_UNSUPPORTED.
 *
 * Errors: fa2_fwd_kvcache_mla_fp8's, and FA2_ERR_BAD_ARG for null indices or index_strides, a negative index stride, topk < 1 and a
 * launch grid that does not fit, and a null k_descale or v_descale with an fp8 cache; all before any launch.
 */
int fa2_fwd_kvcache_mla_sparse(const void *Q, const void *K, const void *V, void *O, void *L,
                               const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                               const int64_t o_strides[4], const int64_t l_strides[2], const int32_t *cache_seqlens,
                               const int32_t *indices, const int64_t index_strides[4], int32_t topk,
                               const int32_t *block_table, int64_t block_table_stride,
                               const float *k_descale, const float *v_descale,
                               const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                               int32_t B, int32_t H, int32_t H_kv, int32_t N_q,
                               int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                               int32_t dtype_enum, int32_t kv_dtype_enum,
                               float scale, int32_t num_splits,
                               void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/* What num_splits = 0 resolves to for it: fa2_kvcache_mla_num_splits' rule with topk in S_k's place and, for f16 / bf16 at d 576 /
 * d_v 512, B * N_q * H_kv * ceil((H / H_kv) / 64) unsplit workgroups: 1 when that is 256 or more, else enough splits for one
 * workgroup per CU, every split at least 4 tiles (256 slots) of the list.  Any other shape is counted as the VALU form's,
 * B * N_q * H_kv * ceil((H / H_kv) / 16) workgroups under fa2_kvcache_num_splits' constants. */
int32_t fa2_kvcache_mla_sparse_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t topk, int32_t d, int32_t d_v,
                                          int32_t dtype_enum);

/*
 * Sparse MLA decode of packed (ragged) queries: fa2_fwd_kvcache_mla_sparse over the packed tensors of fa2_fwd_kvcache_mla_varlen -- a
 * prefill chunk beside one-token decodes, or draft tokens of a different count per sequence, in one call.
 *
 *   Tensors.  Q (total_q, H, d), O (total_q, H, d_v) with three element strides {token, head, column}, L (H, total_q) with unit token
 *             stride and l_head_stride; cu_seqlens_q int32 on the device, B + 1 entries, and max_seqlen_q as in
 *             fa2_fwd_kvcache_mla_varlen: sequence b owns min(clamp(cu[b + 1]) - clamp(cu[b]), max_seqlen_q) rows from clamp(cu[b])
 *             on, the clamp to [0, total_q]; none is legal.  K, V, cache_seqlens, block_table, the descales: fa2_fwd_kvcache_mla_sparse's.
 *   Indices.  int32 on the device, (total_q, H_kv, topk) with three element strides {token, KV head, slot}, each >= 0, 0 allowed.
 *             Entry [t, hk, s] is a logical key position of THE SEQUENCE THAT OWNS packed row t; it is no key when < 0 or
 *             >= N_k(b) of that sequence.  Duplicates, a row without a valid entry (O = 0, L = +inf), the splits over the slots, the
 *             fp8 cache with its required descales and the block table of any page size are fa2_fwd_kvcache_mla_sparse's.
 *   Rows.     Row t belongs to the last sequence b in [0, B) whose clamped offset is <= t, if t lies in that sequence's rows.  A row
 *             no sequence owns -- at or past the clamped cu_seqlens_q[B], or past max_seqlen_q within its sequence -- is neither
 *             read nor written, in O, L and the workspace alike: what fa2_fwd_kvcache_mla_varlen does with it.  Offsets that do not
 *             ascend may give wrong results; every address formed lies inside the tensors for any contents of cu_seqlens_q.
 *   Splits.   The workspace holds fa2_kvcache_varlen_workspace_bytes(total_q, H, d_v, num_splits) bytes; num_splits = 0 resolves to
 *             fa2_kvcache_mla_sparse_varlen_num_splits(...).
 *   Variants. As fa2_fwd_kvcache_mla_sparse: a workgroup owns 64 (GENERIC: 16) heads of one (packed row, KV head).
 *
 * Errors: fa2_fwd_kvcache_mla_sparse's and the packed call's (null cu_seqlens_q, total_q < 1, max_seqlen_q outside [1, 2^28]), all
 * before any launch.
 */
int fa2_fwd_kvcache_mla_sparse_varlen(const void *Q, const void *K, const void *V, void *O, void *L,
                                      const int64_t q_strides[3], const int64_t k_strides[4], const int64_t v_strides[4],
                                      const int64_t o_strides[3], int64_t l_head_stride,
                                      const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                                      const int32_t *indices, const int64_t index_strides[3], int32_t topk,
                                      const int32_t *block_table, int64_t block_table_stride,
                                      const float *k_descale, const float *v_descale,
                                      const int64_t k_descale_strides[2], const int64_t v_descale_strides[2],
                                      int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q,
                                      int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                                      int32_t dtype_enum, int32_t kv_dtype_enum,
                                      float scale, int32_t num_splits,
                                      void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/* What num_splits = 0 resolves to for it: fa2_kvcache_mla_sparse_num_splits with total_q tokens in B * N_q's place.  The workgroup
 * count does not depend on how the tokens fall into sequences: a workgroup owns the heads of one packed row. */
int32_t fa2_kvcache_mla_sparse_varlen_num_splits(int32_t total_q, int32_t H, int32_t H_kv, int32_t topk, int32_t d, int32_t d_v,
                                                 int32_t dtype_enum);

/*
 * The MLA indexer (DeepSeek-V3.2's lightning indexer): the stage in front of fa2_fwd_kvcache_mla_sparse.  It scores every cached
 * token against every query token and makes the key lists that call takes.  Three entry points: the scores alone, the selection
 * alone over any fp32 logits, and both on one stream.
 *
 *   Tensors.  q_idx (B, H_I, N_q, d_I), four element strides; weights fp32 (B, H_I, N_q), three element strides (any softmax or
 *             head scale already folded in); the index-key cache k_idx (B, S_k, d_I) -- one shared head, as the latent cache -- or,
 *             with block_table, the pool (num_blocks, page_size, d_I), k_strides = {batch or block, row, column}; k_scale fp32
 *             (B, S_k) or (num_blocks, page_size), addressed like the rows, k_scale_strides = {batch or block, row}.  Key j of
 *             sequence b in a pool is row j % page_size of page block_table[b, j / page_size], the entry clamped into the pool, ANY
 *             page size; the capacity max_blocks * page_size takes S_k's place.  cache_seqlens as everywhere: null = S_k, clamped.
 *   Dtypes.   q_idx f16, bf16 or f32; k_idx alike, or e4m3fn / e5m2 under f16 / bf16 (storage only: bytes are converted exactly,
 *             the arithmetic stays 16-bit).  k_scale > 0 is optional over a 16-bit or f32 cache and required over an fp8 one.
 *   Scores.   logit[b, qi, j] = k_scale[b, j] * sum_h weights[b, h, qi] * max(0, q_idx[b, h, qi, :] . k_idx[b, j, :]), fp32.
 *   Mask.     Query qi stands at position p = N_k(b) - N_q + qi (bottom-right).  causal != 0: its candidates are the keys
 *             0 .. min(p, N_k(b) - 1), none for p < 0; causal == 0: all N_k(b) keys.  n(b, qi) is their count.
 *   Logits.   fp32 (B, N_q, S_k) at three element strides.  Entry [b, qi, j] is written for j < n(b, qi); no other entry is written
 *             by the score kernels or read by the selection.
 *   Lists.    Values compare as numbers (-0.0 == +0.0, a NaN ranks as -inf).  The list of (b, qi) is the min(topk, n) candidates
 *             that come first under (value descending, position ascending), EMITTED IN ASCENDING POSITION into
 *             indices[b, qi, 0 .. topk), the rest of the row -1; with n <= topk it is 0 .. n - 1 and no logit is read.  indices is
 *             int32 (B, N_q, topk) at three element strides -- the three-dimensional form fa2_fwd_kvcache_mla_sparse's Python
 *             surface takes.  A function of the logits alone: the same logits give the same bytes.
 *   Variants. FA2_INDEXER_VARIANT_IDX16: f16 / bf16 (the cache alike or fp8), d_I = 128, H_I <= 64, unit column strides, 16-byte
 *             aligned rows, contiguous or paged, on v_mfma_f32_16x16x32.  FA2_INDEXER_VARIANT_GENERIC: everything else, on the VALU.
 *             AUTO: IDX16 where it runs, else GENERIC.  A forced IDX16 on a problem it cannot run returns FA2_ERR_UNSUPPORTED.
 *
 * FA2_ERR_BAD_ARG before any launch, the message naming the argument, for: a null q_idx / weights / k_idx / logits (indices) or
 * stride array, a negative stride, B outside [1, 65535], H_I < 1, N_q or S_k outside [1, 2^28], the paged sizes of
 * fa2_fwd_kvcache_paged, topk outside [1, 2^28], an fp8 cache without k_scale, k_scale without its strides, a launch grid that does
 * not fit.  FA2_ERR_UNSUPPORTED for d_I outside [1, 576], a dtype_enum that is not f16 / bf16 / f32, a k_dtype_enum that is neither
 * dtype_enum nor an fp8 format, fp8 under f32, an unknown variant.
 */
#define FA2_INDEXER_VARIANT_AUTO 0
#define FA2_INDEXER_VARIANT_GENERIC 1
#define FA2_INDEXER_VARIANT_IDX16 2

int fa2_mla_indexer_logits(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                           const int64_t q_strides[4], const int64_t w_strides[3], const int64_t k_strides[3],
                           const int64_t k_scale_strides[2], const int64_t logit_strides[3], const int32_t *cache_seqlens,
                           const int32_t *block_table, int64_t block_table_stride,
                           int32_t B, int32_t H_I, int32_t N_q, int32_t S_k, int32_t num_blocks, int32_t page_size,
                           int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum, int32_t causal,
                           int32_t variant, void *hip_stream);

/* The selection alone, over any fp32 logits (B, N_q, S_k): one workgroup per (b, qi) row, a radix select over an order-preserving
 * 32-bit image of the values, then one ordered compaction pass. */
int fa2_topk_indices(const float *logits, const int64_t logit_strides[3], const int32_t *cache_seqlens,
                     int32_t B, int32_t N_q, int32_t S_k, int32_t topk, int32_t causal,
                     int32_t *indices, const int64_t index_strides[3], void *hip_stream);

/* Both on one stream: fa2_mla_indexer_logits into the caller's `logits` buffer (fa2_mla_indexer_workspace_bytes(B, N_q, capacity)
 * bytes when contiguous), then fa2_topk_indices over it.  Every error of both halves comes back before any launch. */
int fa2_mla_indexer_topk(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                         const int64_t q_strides[4], const int64_t w_strides[3], const int64_t k_strides[3],
                         const int64_t k_scale_strides[2], const int64_t logit_strides[3], const int32_t *cache_seqlens,
                         const int32_t *block_table, int64_t block_table_stride,
                         int32_t B, int32_t H_I, int32_t N_q, int32_t S_k, int32_t num_blocks, int32_t page_size,
                         int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum, int32_t causal,
                         int32_t topk, int32_t *indices, const int64_t index_strides[3], int32_t variant, void *hip_stream);

/* Bytes of the contiguous fp32 logits buffer (B, N_q, S_k): 4 * B * N_q * S_k, 0 if a size is < 1, INT64_MAX where that product
 * does not fit. */
int64_t fa2_mla_indexer_workspace_bytes(int32_t B, int32_t N_q, int32_t S_k);

/*
 * The MLA indexer over packed (ragged) queries: the three entry points above for the packed step fa2_fwd_kvcache_mla_sparse_varlen
 * takes.  cu_seqlens_q (int32 on the device, B + 1 entries) and max_seqlen_q are fa2_fwd_kvcache_mla_varlen's: sequence b owns
 * n_q(b) = min(clamp(cu[b + 1]) - clamp(cu[b]), max_seqlen_q) rows from clamp(cu[b]) on, none is legal.
 *
 *   Tensors.  q_idx (total_q, H_I, d_I) with three element strides {token, head, column}; weights fp32 (total_q, H_I), two strides
 *             {token, head}; logits fp32 (total_q, S_k), two strides {row, column}; indices int32 (total_q, topk), two strides
 *             {row, slot} -- the two-dimensional form fa2_fwd_kvcache_mla_sparse_varlen's Python surface expands over the KV heads.
 *             k_idx, k_scale, cache_seqlens and block_table are the fixed calls'.
 *   Mask.     Query i of sequence b stands at position N_k(b) - n_q(b) + i; its candidate count n is the fixed call's with n_q(b)
 *             in N_q's place.
 *   Rows.     The score kernels walk the sequences (a query block of 8 positions lies inside one sequence), the selection takes one
 *             workgroup per packed row and finds its owner as fa2_fwd_kvcache_mla_sparse_varlen does.  A row no sequence owns is
 *             neither scored nor selected: nothing of its logits row or its list is written.
 *   The formula of the logits, which entries are written, the order and tie rule of the lists, the -1 padding and "a function of the
 *   logits alone" are the fixed calls': sequence b of a packed call gives the bytes the fixed call gives on that sequence alone.
 *
 * Errors: the fixed calls' (N_q's range is max_seqlen_q's), and FA2_ERR_BAD_ARG for a null cu_seqlens_q and total_q outside
 * [1, 2^28]; all before any launch.
 */
int fa2_mla_indexer_logits_varlen(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                                  const int64_t q_strides[3], const int64_t w_strides[2], const int64_t k_strides[3],
                                  const int64_t k_scale_strides[2], const int64_t logit_strides[2],
                                  const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                                  const int32_t *block_table, int64_t block_table_stride,
                                  int32_t B, int32_t H_I, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks,
                                  int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum,
                                  int32_t causal, int32_t variant, void *hip_stream);

int fa2_topk_indices_varlen(const float *logits, const int64_t logit_strides[2], const int32_t *cu_seqlens_q,
                            const int32_t *cache_seqlens, int32_t B, int32_t total_q, int32_t max_seqlen_q, int32_t S_k,
                            int32_t topk, int32_t causal, int32_t *indices, const int64_t index_strides[2], void *hip_stream);

int fa2_mla_indexer_topk_varlen(const void *q_idx, const float *weights, const void *k_idx, const float *k_scale, float *logits,
                                const int64_t q_strides[3], const int64_t w_strides[2], const int64_t k_strides[3],
                                const int64_t k_scale_strides[2], const int64_t logit_strides[2],
                                const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                                const int32_t *block_table, int64_t block_table_stride,
                                int32_t B, int32_t H_I, int32_t total_q, int32_t max_seqlen_q, int32_t S_k, int32_t num_blocks,
                                int32_t page_size, int32_t max_blocks, int32_t d_I, int32_t dtype_enum, int32_t k_dtype_enum,
                                int32_t causal, int32_t topk, int32_t *indices, const int64_t index_strides[2], int32_t variant,
                                void *hip_stream);

/* Bytes of the contiguous fp32 logits buffer (total_q, S_k): 4 * total_q * S_k, 0 if a size is < 1. */
int64_t fa2_mla_indexer_varlen_workspace_bytes(int32_t total_q, int32_t S_k);

/*
 * The fused ragged MLA step: fa2_kvcache_mla_append_varlen over cu_seqlens_q (total_new = total_q, max_seqlen_new = max_seqlen_q;
 * c_new, pe_new packed (total_q, H_kv, d_v) / (total_q, H_kv, d - d_v)), then on the same stream fa2_fwd_kvcache_mla_varlen over the
 * updated cache with seqlens_out as its cache_seqlens and, with tables, q_rot (packed, contiguous (total_q, H, d)) as its Q; q_rot
 * may be null without them.  q_pos_per_row is causal || window_left >= 0 || window_right >= 0.  cache_seqlens holds the lengths
 * BEFORE the append and is not modified.  Every error of both halves comes back before any launch, and a forced
 * FA2_KVCACHE_VARIANT_MLA16 that cannot run the problem fails before the cache is written.
 */
int fa2_fwd_kvcache_mla_varlen_append(const void *Q, void *KV, void *O, void *L,
                                      const int64_t q_strides[3], const int64_t kv_strides[4], const int64_t o_strides[3],
                                      int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cache_seqlens,
                                      int32_t *seqlens_out, const int32_t *block_table, int64_t block_table_stride,
                                      const float *kv_descale, const int64_t kv_descale_strides[2],
                                      const void *c_new, const void *pe_new, const int64_t c_new_strides[3],
                                      const int64_t pe_new_strides[3],
                                      const void *rotary_cos, const void *rotary_sin, int64_t rotary_cos_stride,
                                      int64_t rotary_sin_stride, int32_t S_rot, int32_t rotary_dim, int32_t rotary_interleaved,
                                      void *q_rot, int32_t B, int32_t H, int32_t H_kv, int32_t total_q, int32_t max_seqlen_q,
                                      int32_t S_k, int32_t num_blocks, int32_t page_size, int32_t max_blocks, int32_t d, int32_t d_v,
                                      int32_t dtype_enum, int32_t kv_dtype_enum,
                                      int32_t causal, float scale, int32_t window_left, int32_t window_right, int32_t num_splits,
                                      void *workspace, int64_t workspace_bytes, int32_t variant, void *hip_stream);

/* Bytes of workspace a call with this num_splits needs: 0 for num_splits <= 1, else fp32 partial O of num_splits * B * H * N_q * d
 * elements plus fp32 partial L of num_splits * B * H * N_q. */
int64_t fa2_kvcache_workspace_bytes(int32_t B, int32_t H, int32_t N_q, int32_t d, int32_t num_splits);

/* What num_splits = 0 resolves to, in [1, FA2_KVCACHE_MAX_SPLITS]: 1 when the unsplit launch already has 256 workgroups, else enough
 * splits for two workgroups per CU, every split at least 4 key tiles (256 keys) of the capacity S_k.  The unsplit launch is counted
 * for the form AUTO takes as far as the shape decides it: B * H_kv workgroups for f16 / bf16 at d 64 / 128 with
 * (H / H_kv) * N_q <= 64 (the matrix form), B * H * ceil(N_q / 16) otherwise (the VALU form); strides and alignment are not seen. */
int32_t fa2_kvcache_num_splits(int32_t B, int32_t H, int32_t H_kv, int32_t N_q, int32_t S_k, int32_t d, int32_t dtype_enum);

/* Which tile the static table picks for a contiguous problem: out4 = {variant, B_r, B_c, waves}.
 * Counterpart of fwd_conf_prune + the autotuner's choice (src/autotune_configs.py:176-194). */
int fa2_query_tile(int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, int32_t out4[4]);

/* The table's choice depends on the grid size (B * H tiles must fill 256 CUs): fa2_query_tile answers for a large grid
 * (B = 64, H = 8), fa2_query_tile_ex for the given B and H -- the variant fa2_fwd() runs for that contiguous problem at
 * scale = 1 (the reference's). */
int fa2_query_tile_ex(int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                      int32_t out4[4]);

/* ... and for a given softmax scale: f16 rescales its accumulators every few key tiles at the reference's scale of 1 (P must stay
 * below 65 504) and hardly ever at the usual 1 / sqrt(d), which moves two of the table's thresholds (fa2_api.hip). */
int fa2_query_tile_scaled(int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                          int32_t out4[4]);

/* "fa2-hip <semver> gfx950". */
const char *fa2_version(void);

/* Message of the last non-zero return on the calling thread ("" if none). */
const char *fa2_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FA2_FWD_H */
