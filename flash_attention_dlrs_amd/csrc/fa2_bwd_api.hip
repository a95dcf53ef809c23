// fa2_bwd_api.hip -- extern "C" entry points of the backward (declared in include/fa2_bwd.h).
#include <string.h>

#include "fa2_bwd_common.h"

namespace {

bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

int validate(const Fa2BwdProblem &p) {
    if (!p.Q || !p.K || !p.V || !p.O || !p.dO || !p.L || !p.dQ || !p.dK || !p.dV || !p.D) {
        fa2_set_error("null tensor pointer");
        return FA2_ERR_BAD_ARG;
    }
    if (p.B <= 0 || p.H <= 0 || p.d <= 0) {
        fa2_set_error("B, H, d must be positive (got B=%d H=%d d=%d)", p.B, p.H, p.d);
        return FA2_ERR_BAD_ARG;
    }
    if (p.N < 1) {
        fa2_set_error("N must be >= 1 (got %d)", p.N);
        return FA2_ERR_BAD_N;
    }
    if (p.dtype != FA2_DTYPE_F32 && p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16 && p.dtype != FA2_DTYPE_F64) {
        fa2_set_error("backward: dtype enum %d is not supported (f64, f32, f16, bf16)", p.dtype);
        return FA2_ERR_UNSUPPORTED;
    }
    if (!is_pow2(p.d) || p.d < 16 || p.d > 512) {  // the glue pads d exactly as in the forward (torch.py:95-99)
        fa2_set_error("d=%d must be a power of two in [16, 512] (pad on the host as the reference does)", p.d);
        return FA2_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < 4; ++k)
        if (p.qs[k] < 0 || p.ks[k] < 0 || p.vs[k] < 0 || p.os[k] < 0 || p.dos[k] < 0 || p.dqs[k] < 0 || p.dks[k] < 0 || p.dvs[k] < 0) {
            fa2_set_error("negative strides are not supported");
            return FA2_ERR_BAD_ARG;
        }
    if (p.dqs[3] == 0 || p.dks[3] == 0 || p.dvs[3] == 0 || (p.N > 1 && (p.dqs[2] == 0 || p.dks[2] == 0 || p.dvs[2] == 0))) {
        fa2_set_error("dQ, dK, dV must not alias themselves (zero stride)");
        return FA2_ERR_BAD_ARG;
    }
    if (!(p.scale == p.scale)) {
        fa2_set_error("scale is NaN");
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

int run(const Fa2BwdProblem &p, int variant) {
    const int rc = validate(p);
    if (rc != FA2_OK) return rc;
    if (variant == FA2_BWD_VARIANT_AUTO)
        variant = fa2_bwd_mfma16_supports(p)   ? FA2_BWD_VARIANT_MFMA16
                  : fa2_bwd_mfma32_supports(p) ? FA2_BWD_VARIANT_MFMA32
                                               : FA2_BWD_VARIANT_GENERIC;
    switch (variant) {
    case FA2_BWD_VARIANT_GENERIC: return fa2_bwd_launch_generic(p);
    case FA2_BWD_VARIANT_MFMA16: return fa2_bwd_launch_mfma16(p);
    case FA2_BWD_VARIANT_MFMA32: return fa2_bwd_launch_mfma32(p);
    default: fa2_set_error("unknown backward kernel variant %d", variant); return FA2_ERR_BAD_ARG;
    }
}

// Windowed backward (fa2_bwd_window): the MFMA kernel for f16 / bf16 at d = 64 / 128, the VALU kernel for the rest.
int run_window(const Fa2BwdProblem &p, int variant) {
    const int rc = validate(p);
    if (rc != FA2_OK) return rc;
    if (variant == FA2_BWD_VARIANT_AUTO) variant = fa2_bwd_mfma16_supports(p) ? FA2_BWD_VARIANT_MFMA16 : FA2_BWD_VARIANT_GENERIC;
    switch (variant) {
    case FA2_BWD_VARIANT_GENERIC: return fa2_bwd_launch_generic_window(p);
    case FA2_BWD_VARIANT_MFMA16: return fa2_bwd_launch_mfma16_window(p);
    default:
        fa2_set_error("backward kernel variant %d does not take a window (generic and mfma16 do)", variant);
        return FA2_ERR_UNSUPPORTED;
    }
}

Fa2BwdProblem make(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                   void *dK, void *dV, void *D, const int64_t *qs, const int64_t *ks, const int64_t *vs,
                   const int64_t *os, const int64_t *dos, const int64_t *dqs, const int64_t *dks, const int64_t *dvs,
                   const int64_t *ls, int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype, int32_t causal,
                   float scale, void *stream) {
    Fa2BwdProblem p;
    memset(&p, 0, sizeof(p));
    p.Q = Q; p.K = K; p.V = V; p.O = O; p.dO = dO; p.L = L;
    p.dQ = dQ; p.dK = dK; p.dV = dV; p.D = D;
    if (qs && ks && vs && os && dos && dqs && dks && dvs && ls) {
        for (int k = 0; k < 4; ++k) {
            p.qs[k] = qs[k]; p.ks[k] = ks[k]; p.vs[k] = vs[k]; p.os[k] = os[k]; p.dos[k] = dos[k];
            p.dqs[k] = dqs[k]; p.dks[k] = dks[k]; p.dvs[k] = dvs[k];
        }
        p.ls[0] = ls[0]; p.ls[1] = ls[1];
    } else {
        p.Q = nullptr;  // fails validate()
    }
    p.B = B; p.H = H; p.N = N; p.d = d; p.dtype = dtype; p.causal = causal ? 1 : 0; p.scale = scale;
    p.stream = (hipStream_t)stream;
    return p;
}

int bwd_window(Fa2BwdProblem p, int32_t wl, int32_t wr, int variant) {
    int32_t c = p.causal, l = 0, r = 0, windowed = 0;
    if (p.N >= 1) {  // (N < 1 is reported by validate())
        const int rc = fa2_window_normalise(p.N, p.causal, wl, wr, &c, &l, &r, &windowed);
        if (rc != FA2_OK) return rc;
    } else if (wl < -1 || wr < -1) {
        fa2_set_error("window sides must be >= -1 (-1 = unbounded), got window=(%d, %d)", wl, wr);
        return FA2_ERR_BAD_ARG;
    }
    p.causal = c;
    if (!windowed) return run(p, variant);  // the window removes nothing beyond plain / causal attention: the same path
    p.causal = 0;
    p.wl = l;
    p.wr = r;
    return run_window(p, variant);
}

// Variable-length (packed) backward, fa2_bwd_varlen: arguments checked before any launch.
int bwd_varlen(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ, void *dK, void *dV,
               void *D, const int64_t *const st3[8], int64_t l_head_stride, const int32_t *cu_q, const int32_t *cu_k, int32_t B,
               int32_t H, int32_t d, int32_t max_q, int32_t max_k, int32_t total_q, int32_t total_k, int32_t dtype, int32_t causal,
               float scale, int32_t wl, int32_t wr, void *stream, int variant, int gqa = 1) {
    const char *snames[8] = {"q_strides", "k_strides", "v_strides", "o_strides", "do_strides", "dq_strides", "dk_strides", "dv_strides"};
    for (int t = 0; t < 8; ++t)
        if (!st3[t]) {
            fa2_set_error("varlen backward: null %s", snames[t]);
            return FA2_ERR_BAD_ARG;
        }
    if (!cu_q || !cu_k) {
        fa2_set_error("varlen backward: null %s", !cu_q ? "cu_seqlens_q" : "cu_seqlens_k");
        return FA2_ERR_BAD_ARG;
    }
    if (B < 1 || B > 65535) {
        fa2_set_error("varlen backward: B (number of sequences) must be in [1, 65535] (got %d)", B);
        return FA2_ERR_BAD_ARG;
    }
    if (H > 65535) {
        fa2_set_error("varlen backward: H must be <= 65535 (got %d)", H);
        return FA2_ERR_BAD_ARG;
    }
    if (max_q < 0 || max_k < 0 || max_q > (1 << 28) || max_k > (1 << 28)) {
        fa2_set_error("varlen backward: max_seqlen_q and max_seqlen_k must be in [0, 2^28] (got %d, %d)", max_q, max_k);
        return FA2_ERR_BAD_ARG;
    }
    if (total_q < 0 || total_k < 0) {
        fa2_set_error("varlen backward: total_q and total_k must be >= 0 (got %d, %d)", total_q, total_k);
        return FA2_ERR_BAD_ARG;
    }
    if (wl < -1 || wr < -1) {
        fa2_set_error("window sides must be >= -1 (-1 = unbounded), got window=(%d, %d)", wl, wr);
        return FA2_ERR_BAD_ARG;
    }
    if (l_head_stride < 0) {
        fa2_set_error("varlen backward: negative L head stride");
        return FA2_ERR_BAD_ARG;
    }
    const void *ptrs[10] = {Q, K, V, O, dO, L, dQ, dK, dV, D};
    const char *names[10] = {"Q", "K", "V", "O", "dO", "L", "dQ", "dK", "dV", "D"};
    for (int t = 0; t < 10; ++t)
        if (!ptrs[t]) {
            fa2_set_error("varlen backward: null %s", names[t]);
            return FA2_ERR_BAD_ARG;
        }
    int64_t s4[8][4];
    for (int t = 0; t < 8; ++t) {
        s4[t][0] = 0; s4[t][1] = st3[t][1]; s4[t][2] = st3[t][0]; s4[t][3] = st3[t][2];
    }
    const int64_t ls2[2] = {0, l_head_stride};
    const int32_t nmax = max_q > max_k ? max_q : max_k;
    Fa2BwdProblem p = make(Q, K, V, O, dO, L, dQ, dK, dV, D, s4[0], s4[1], s4[2], s4[3], s4[4], s4[5], s4[6], s4[7], ls2, B, H,
                           nmax > 0 ? nmax : 1, d, dtype, causal, scale, stream);
    const int rc = validate(p);
    if (rc != FA2_OK) return rc;
    p.wl = wl;
    p.wr = wr;
    p.cu_q = cu_q; p.cu_k = cu_k;
    p.max_q = max_q; p.max_k = max_k; p.total_q = total_q; p.total_k = total_k;
    // (fa2_bwd_mfma16_supports judges the 32-bit offsets on N = the longer max_seqlen: they span one sequence)
    if (variant == FA2_BWD_VARIANT_AUTO) variant = fa2_bwd_mfma16_supports(p) ? FA2_BWD_VARIANT_MFMA16 : FA2_BWD_VARIANT_GENERIC;
    if (gqa > 1) {  // grouped-query: K, V, dK, dV carry H / gqa heads
        switch (variant) {
        case FA2_BWD_VARIANT_GENERIC: return fa2_bwd_launch_generic_varlen_gqa(p, gqa);
        case FA2_BWD_VARIANT_MFMA16: return fa2_bwd_launch_mfma16_varlen_gqa(p, gqa);
        default:
            fa2_set_error("backward kernel variant %d has no varlen GQA form (generic and mfma16 do)", variant);
            return FA2_ERR_UNSUPPORTED;
        }
    }
    switch (variant) {
    case FA2_BWD_VARIANT_GENERIC: return fa2_bwd_launch_generic_varlen(p);
    case FA2_BWD_VARIANT_MFMA16: return fa2_bwd_launch_mfma16_varlen(p);
    default:
        fa2_set_error("backward kernel variant %d has no varlen form (generic and mfma16 do)", variant);
        return FA2_ERR_UNSUPPORTED;
    }
}

// Grouped-query backward, dense layout (fa2_bwd_gqa).  H_kv == H is fa2_bwd_window itself.  Otherwise the windowed GQA forms, with a
// plain or causal problem as the full band (its arithmetic is the plain kernels': the same sweep, the same masks), sum dK / dV of
// each KV head over its g query heads inside one workgroup.
int bwd_gqa(Fa2BwdProblem p, int32_t H_kv, int32_t wl, int32_t wr, int variant) {
    int rc = fa2_check_gqa(p.H, H_kv);
    if (rc != FA2_OK) return rc;
    if (H_kv == p.H) return bwd_window(p, wl, wr, variant);
    int32_t c = p.causal, l = 0, r = 0, windowed = 0;
    if (p.N >= 1) {  // (N < 1 is reported by validate())
        rc = fa2_window_normalise(p.N, p.causal, wl, wr, &c, &l, &r, &windowed);
        if (rc != FA2_OK) return rc;
    } else if (wl < -1 || wr < -1) {
        fa2_set_error("window sides must be >= -1 (-1 = unbounded), got window=(%d, %d)", wl, wr);
        return FA2_ERR_BAD_ARG;
    }
    rc = validate(p);
    if (rc != FA2_OK) return rc;
    p.causal = 0;  // the band carries the mask: (N - 1, N - 1) plain, (N - 1, 0) causal
    p.wl = l;
    p.wr = r;
    const int g = p.H / H_kv;
    if (variant == FA2_BWD_VARIANT_AUTO) variant = fa2_bwd_mfma16_supports(p) ? FA2_BWD_VARIANT_MFMA16 : FA2_BWD_VARIANT_GENERIC;
    switch (variant) {
    case FA2_BWD_VARIANT_GENERIC: return fa2_bwd_launch_generic_window_gqa(p, g);
    case FA2_BWD_VARIANT_MFMA16: return fa2_bwd_launch_mfma16_window_gqa(p, g);
    default:
        fa2_set_error("backward kernel variant %d has no GQA form (generic and mfma16 do)", variant);
        return FA2_ERR_UNSUPPORTED;
    }
}

}  // namespace

extern "C" {

int fa2_bwd_gqa(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ, void *dK,
                void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4], const int64_t dk_strides[4],
                const int64_t dv_strides[4], const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d,
                int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return bwd_gqa(make(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                        dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream),
                   H_kv, window_left, window_right, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_gqa_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                        void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                        const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                        const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                        const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d, int32_t dtype_enum,
                        int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                        int32_t variant) {
    return bwd_gqa(make(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                        dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream),
                   H_kv, window_left, window_right, variant);
}

int fa2_bwd_varlen_gqa(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                       void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                       const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                       const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                       int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                       int32_t H_kv, int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                       int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                       void *hip_stream) {
    return fa2_bwd_varlen_gqa_variant(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides,
                                      dq_strides, dk_strides, dv_strides, l_head_stride, cu_seqlens_q, cu_seqlens_k, B, H, H_kv, d,
                                      max_seqlen_q, max_seqlen_k, total_q, total_k, dtype_enum, causal, scale, window_left,
                                      window_right, hip_stream, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_varlen_gqa_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                               void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                               const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                               const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                               int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B,
                               int32_t H, int32_t H_kv, int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                               int32_t total_k, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                               int32_t window_right, void *hip_stream, int32_t variant) {
    const int rc = fa2_check_gqa(H, H_kv);
    if (rc != FA2_OK) return rc;
    const int64_t *const st[8] = {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides};
    return bwd_varlen(Q, K, V, O, dO, L, dQ, dK, dV, D, st, l_head_stride, cu_seqlens_q, cu_seqlens_k, B, H, d, max_seqlen_q,
                      max_seqlen_k, total_q, total_k, dtype_enum, causal, scale, window_left, window_right, hip_stream, variant,
                      H >= 1 ? H / H_kv : 1);
}

int fa2_bwd(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
            void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
            const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
            const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
            const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
            float scale, void *hip_stream) {
    return run(make(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                    dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream),
               FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                    void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                    const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                    const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                    const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
                    int32_t causal, float scale, void *hip_stream, int32_t variant) {
    return run(make(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                    dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream),
               variant);
}

int fa2_bwd_window(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                   void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                   const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                   const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                   const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                   float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return bwd_window(make(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream),
                      window_left, window_right, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_window_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                           void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                           const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                           const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                           const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
                           int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                           int32_t variant) {
    return bwd_window(make(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream),
                      window_left, window_right, variant);
}

int fa2_bwd_varlen(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                   void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                   const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                   const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                   const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                   int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t dtype_enum,
                   int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    const int64_t *const st[8] = {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides};
    return bwd_varlen(Q, K, V, O, dO, L, dQ, dK, dV, D, st, l_head_stride, cu_seqlens_q, cu_seqlens_k, B, H, d, max_seqlen_q,
                      max_seqlen_k, total_q, total_k, dtype_enum, causal, scale, window_left, window_right, hip_stream,
                      FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_varlen_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                           void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                           const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                           const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                           int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                           int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                           int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                           void *hip_stream, int32_t variant) {
    const int64_t *const st[8] = {q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides, dk_strides, dv_strides};
    return bwd_varlen(Q, K, V, O, dO, L, dQ, dK, dV, D, st, l_head_stride, cu_seqlens_q, cu_seqlens_k, B, H, d, max_seqlen_q,
                      max_seqlen_k, total_q, total_k, dtype_enum, causal, scale, window_left, window_right, hip_stream, variant);
}

}  // extern "C"
