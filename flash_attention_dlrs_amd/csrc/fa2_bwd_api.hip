// fa2_bwd_api.hip -- extern "C" entry points of the backward (declared in include/fa2_bwd.h).
#include <string.h>

#include "fa2_bwd_common.h"
#include "fa2_host.h"

namespace {

bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// any_d: fa2_bwd_varlen_dv, whose d follows the forward call's rule (nothing pads it)
int validate(const Fa2BwdProblem &p, bool any_d = false) {
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
    if (any_d) {
        if (p.d > 512) {
            fa2_set_error("d=%d must be in [1, 512]", p.d);
            return FA2_ERR_UNSUPPORTED;
        }
    } else if (!is_pow2(p.d) || p.d < 16 || p.d > 512) {  // the glue pads d exactly as in the forward (torch.py:95-99)
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

// The table of the five forms (FA2_FORM_DENSE .. FA2_FORM_VARLEN_GQA): each takes GENERIC and MFMA16 -- AUTO: MFMA16 (f16 / bf16 at
// d = 64 / 128) where it runs, else the VALU kernel -- and refuses any other id with its own sentence.  The dense form alone also
// has MFMA32, and what it refuses is FA2_ERR_BAD_ARG.  (fa2_bwd_mfma16_supports judges the 32-bit offsets of a packed problem on
// N = the longer max_seqlen: they span one sequence.)
using P = const Fa2BwdProblem &;
struct FormRow {
    int (*generic)(P, int g);
    int (*mfma16)(P, int g);
    const char *other;
};
const FormRow kForms[5] = {
    {[](P p, int) { return fa2_bwd_launch_generic(p); }, [](P p, int) { return fa2_bwd_launch_mfma16(p); },
     "unknown backward kernel variant %d"},
    {[](P p, int) { return fa2_bwd_launch_generic_window(p); }, [](P p, int) { return fa2_bwd_launch_mfma16_window(p); },
     "backward kernel variant %d does not take a window (generic and mfma16 do)"},
    {[](P p, int) { return fa2_bwd_launch_generic_varlen(p); }, [](P p, int) { return fa2_bwd_launch_mfma16_varlen(p); },
     "backward kernel variant %d has no varlen form (generic and mfma16 do)"},
    {fa2_bwd_launch_generic_window_gqa, fa2_bwd_launch_mfma16_window_gqa, "backward kernel variant %d has no GQA form (generic and mfma16 do)"},
    {fa2_bwd_launch_generic_varlen_gqa, fa2_bwd_launch_mfma16_varlen_gqa,
     "backward kernel variant %d has no varlen GQA form (generic and mfma16 do)"},
};

// Step 3: the launch of a checked problem in its form.
int run_bwd(const Fa2BwdProblem &p, Fa2Form form, int variant) {
    const bool dense = form.kind == FA2_FORM_DENSE;
    if (variant == FA2_BWD_VARIANT_AUTO)
        variant = fa2_bwd_mfma16_supports(p)            ? FA2_BWD_VARIANT_MFMA16
                  : dense && fa2_bwd_mfma32_supports(p) ? FA2_BWD_VARIANT_MFMA32
                                                        : FA2_BWD_VARIANT_GENERIC;
    const FormRow &row = kForms[form.kind];
    if (variant == FA2_BWD_VARIANT_GENERIC) return row.generic(p, form.g);
    if (variant == FA2_BWD_VARIANT_MFMA16) return row.mfma16(p, form.g);
    if (variant == FA2_BWD_VARIANT_MFMA32 && dense) return fa2_bwd_launch_mfma32(p);
    fa2_set_error(row.other, variant);
    return dense ? FA2_ERR_BAD_ARG : FA2_ERR_UNSUPPORTED;
}

// fa2_bwd_varlen_dv: a checked packed problem with a value head size of its own (p.dv).  At d_v == d it is the varlen (GQA) call
// itself, through the table above; else the matrix kernel where it runs (d 192 / d_v 128, 16-bit) or the VALU form.
int run_bwd_dv(const Fa2BwdProblem &p, Fa2Form form, int variant) {
    if (p.dv == p.d) return run_bwd(p, form, variant);
    if (variant == FA2_BWD_VARIANT_AUTO) variant = fa2_bwd_mfma16dv_supports(p) ? FA2_BWD_VARIANT_MFMA16DV : FA2_BWD_VARIANT_GENERIC;
    if (variant == FA2_BWD_VARIANT_GENERIC) return fa2_bwd_launch_generic_varlen_dv(p, form.g);
    if (variant == FA2_BWD_VARIANT_MFMA16DV) return fa2_bwd_launch_mfma16dv(p, form.g);
    fa2_set_error("backward kernel variant %d is not one of fa2_bwd_varlen_dv's at d_v != d (generic and mfma16dv are)", variant);
    return FA2_ERR_UNSUPPORTED;
}

// Step 1: the raw arguments of any of the twelve backward entry points, as FwdCall (fa2_api.hip) holds the forward's.  `strides`: of
// Q, K, V, O, dO, dQ, dK, dV in that order, 4 elements each, 3 in a packed call.
struct BwdCall {
    const void *Q, *K, *V, *O, *dO, *L;
    void *dQ, *dK, *dV, *D;
    const int64_t *strides[8], *l_strides;
    int32_t B, H, N, d, dtype_enum, causal;
    float scale;
    void *hip_stream;
    int32_t variant;
    int32_t window_left = -1, window_right = -1;
    bool gqa = false;  // fa2_bwd_gqa, fa2_bwd_varlen_gqa: K, V, dK, dV have H_kv heads
    int32_t H_kv = 0;
    bool packed = false;  // fa2_bwd_varlen, fa2_bwd_varlen_gqa
    const int32_t *cu_seqlens_q = nullptr, *cu_seqlens_k = nullptr;
    int32_t max_seqlen_q = 0, max_seqlen_k = 0, total_q = 0, total_k = 0;
    int64_t l_head_stride = 0;
    bool has_dv = false;  // fa2_bwd_varlen_dv (a packed GQA call): V, O, dO, dV have d_v columns
    int32_t d_v = 0;
};

// Step 2: check_fwd's order (tests/golden/train_host_calls.json), with the packed call's own: its stride pointers, sizes and L's
// head stride before its tensors.  Grouped-query attention (H_kv < H) always runs the GQA forms -- a dense problem without a window
// as the full band: the same sweep, the same masks -- which sum dK / dV of each KV head over its g query heads inside one workgroup.
int check_bwd(const BwdCall &c, Fa2BwdProblem &p, Fa2Form &form) {
    form = {FA2_FORM_DENSE, 1};
    if (c.gqa) {
        const int rc = fa2_check_gqa(c.H, c.H_kv);
        if (rc != FA2_OK) return rc;
        if (c.H >= 1) form.g = c.H / c.H_kv;
    }
    memset(&p, 0, sizeof(p));
    p.Q = c.Q; p.K = c.K; p.V = c.V; p.O = c.O; p.dO = c.dO; p.L = c.L;
    p.dQ = c.dQ; p.dK = c.dK; p.dV = c.dV; p.D = c.D;
    p.B = c.B; p.H = c.H; p.d = c.d; p.dtype = c.dtype_enum; p.causal = c.causal ? 1 : 0; p.scale = c.scale;
    p.stream = (hipStream_t)c.hip_stream;
    int64_t *const strides[8] = {p.qs, p.ks, p.vs, p.os, p.dos, p.dqs, p.dks, p.dvs};
    if (c.packed) {
        const char *snames[8] = {"q_strides", "k_strides", "v_strides", "o_strides", "do_strides", "dq_strides", "dk_strides", "dv_strides"};
        int rc = fa2_check_nonnull("varlen backward", (const void *const *)c.strides, snames, 8);
        if (rc == FA2_OK) rc = fa2_check_packed("varlen backward", c, false);
        if (rc != FA2_OK) return rc;
        if (c.l_head_stride < 0) {
            fa2_set_error("varlen backward: negative L head stride");
            return FA2_ERR_BAD_ARG;
        }
        const void *ptrs[10] = {c.Q, c.K, c.V, c.O, c.dO, c.L, c.dQ, c.dK, c.dV, c.D};
        const char *names[10] = {"Q", "K", "V", "O", "dO", "L", "dQ", "dK", "dV", "D"};
        rc = fa2_check_nonnull("varlen backward", ptrs, names, 10);
        if (rc != FA2_OK) return rc;
        for (int t = 0; t < 8; ++t) fa2_packed_strides4(c.strides[t], strides[t]);
        fa2_set_packed(c, p);
        form.kind = form.g > 1 ? FA2_FORM_VARLEN_GQA : FA2_FORM_VARLEN;
        rc = validate(p, c.has_dv);
        if (rc != FA2_OK || !c.has_dv) return rc;
        if (c.d_v < 1 || c.d_v > 512) {  // (after every check of fa2_bwd_varlen_gqa, as check_fwd orders it)
            fa2_set_error("varlen backward: d_v=%d must be in [1, 512]", c.d_v);
            return FA2_ERR_BAD_ARG;
        }
        p.dv = c.d_v;
        return FA2_OK;
    }
    Fa2Window w;
    int rc = fa2_window_of(c.N, c.causal, c.window_left, c.window_right, w);
    if (rc != FA2_OK) return rc;
    bool all = c.l_strides;
    for (int t = 0; t < 8; ++t) all = all && c.strides[t];
    if (all) {
        for (int t = 0; t < 8; ++t)
            for (int k = 0; k < 4; ++k) strides[t][k] = c.strides[t][k];
        p.ls[0] = c.l_strides[0]; p.ls[1] = c.l_strides[1];
    } else {
        p.Q = nullptr;  // fails validate()
    }
    p.N = c.N;
    p.causal = w.causal;
    rc = validate(p);
    if (rc != FA2_OK) return rc;
    if (w.windowed || form.g > 1) {  // the band carries the mask; a GQA call's always: (N - 1, N - 1) plain, (N - 1, 0) causal
        form.kind = form.g > 1 ? FA2_FORM_WINDOW_GQA : FA2_FORM_WINDOW;
        p.causal = 0;
        p.wl = w.wl;
        p.wr = w.wr;
    }
    return FA2_OK;
}

int bwd(const BwdCall &c) {
    Fa2BwdProblem p;
    Fa2Form form;
    const int rc = check_bwd(c, p, form);
    if (rc != FA2_OK) return rc;
    return c.has_dv ? run_bwd_dv(p, form, c.variant) : run_bwd(p, form, c.variant);
}

// What every entry point fills alike (a packed one: 3-element strides, no l_strides, no N); the rest each adds its own.
BwdCall dense_call(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ, void *dK, void *dV,
                   void *D, const int64_t *qs, const int64_t *ks, const int64_t *vs, const int64_t *os, const int64_t *dos,
                   const int64_t *dqs, const int64_t *dks, const int64_t *dvs, const int64_t *ls, int32_t B, int32_t H, int32_t N,
                   int32_t d, int32_t dtype_enum, int32_t causal, float scale, void *hip_stream, int32_t variant) {
    BwdCall c = {Q, K, V, O, dO, L, dQ, dK, dV, D, {qs, ks, vs, os, dos, dqs, dks, dvs}, ls};
    c.B = B; c.H = H; c.N = N; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale; c.hip_stream = hip_stream;
    c.variant = variant;
    return c;
}

}  // namespace

// Every entry point fills a call and hands it to bwd(); X is X_variant with FA2_BWD_VARIANT_AUTO.
extern "C" {

int fa2_bwd(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
            void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
            const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
            const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
            const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
            float scale, void *hip_stream) {
    return fa2_bwd_variant(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                    void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                    const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                    const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                    const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
                    int32_t causal, float scale, void *hip_stream, int32_t variant) {
    return bwd(dense_call(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                          dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream, variant));
}

int fa2_bwd_window(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                   void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                   const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                   const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                   const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                   float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_bwd_window_variant(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                                  dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, window_left, window_right,
                                  hip_stream, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_window_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                           void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                           const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                           const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                           const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
                           int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                           int32_t variant) {
    BwdCall c = dense_call(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream, variant);
    c.window_left = window_left; c.window_right = window_right;
    return bwd(c);
}

int fa2_bwd_gqa(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ, void *dK,
                void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4], const int64_t v_strides[4],
                const int64_t o_strides[4], const int64_t do_strides[4], const int64_t dq_strides[4], const int64_t dk_strides[4],
                const int64_t dv_strides[4], const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d,
                int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_bwd_gqa_variant(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                               dk_strides, dv_strides, l_strides, B, H, H_kv, N, d, dtype_enum, causal, scale, window_left,
                               window_right, hip_stream, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_gqa_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                        void *dK, void *dV, void *D, const int64_t q_strides[4], const int64_t k_strides[4],
                        const int64_t v_strides[4], const int64_t o_strides[4], const int64_t do_strides[4],
                        const int64_t dq_strides[4], const int64_t dk_strides[4], const int64_t dv_strides[4],
                        const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d, int32_t dtype_enum,
                        int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                        int32_t variant) {
    BwdCall c = dense_call(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, l_strides, B, H, N, d, dtype_enum, causal, scale, hip_stream, variant);
    c.window_left = window_left; c.window_right = window_right;
    c.gqa = true; c.H_kv = H_kv;
    return bwd(c);
}

int fa2_bwd_varlen(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                   void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                   const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                   const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3], int64_t l_head_stride,
                   const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                   int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t dtype_enum,
                   int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_bwd_varlen_variant(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                                  dk_strides, dv_strides, l_head_stride, cu_seqlens_q, cu_seqlens_k, B, H, d, max_seqlen_q, max_seqlen_k,
                                  total_q, total_k, dtype_enum, causal, scale, window_left, window_right, hip_stream,
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
    BwdCall c = dense_call(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, nullptr, B, H, 0, d, dtype_enum, causal, scale, hip_stream, variant);
    fa2_call_packed(c, l_head_stride, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, total_q, total_k, window_left, window_right);
    return bwd(c);
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
    BwdCall c = dense_call(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, nullptr, B, H, 0, d, dtype_enum, causal, scale, hip_stream, variant);
    fa2_call_packed(c, l_head_stride, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, total_q, total_k, window_left, window_right);
    c.gqa = true; c.H_kv = H_kv;
    return bwd(c);
}

int fa2_bwd_varlen_dv(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L, void *dQ,
                      void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                      const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                      const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                      int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                      int32_t H_kv, int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                      int32_t total_k, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                      void *hip_stream) {
    return fa2_bwd_varlen_dv_variant(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides,
                                     dq_strides, dk_strides, dv_strides, l_head_stride, cu_seqlens_q, cu_seqlens_k, B, H, H_kv, d, d_v,
                                     max_seqlen_q, max_seqlen_k, total_q, total_k, dtype_enum, causal, scale, window_left,
                                     window_right, hip_stream, FA2_BWD_VARIANT_AUTO);
}

int fa2_bwd_varlen_dv_variant(const void *Q, const void *K, const void *V, const void *O, const void *dO, const void *L,
                              void *dQ, void *dK, void *dV, void *D, const int64_t q_strides[3], const int64_t k_strides[3],
                              const int64_t v_strides[3], const int64_t o_strides[3], const int64_t do_strides[3],
                              const int64_t dq_strides[3], const int64_t dk_strides[3], const int64_t dv_strides[3],
                              int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B,
                              int32_t H, int32_t H_kv, int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k,
                              int32_t total_q, int32_t total_k, int32_t dtype_enum, int32_t causal, float scale,
                              int32_t window_left, int32_t window_right, void *hip_stream, int32_t variant) {
    BwdCall c = dense_call(Q, K, V, O, dO, L, dQ, dK, dV, D, q_strides, k_strides, v_strides, o_strides, do_strides, dq_strides,
                           dk_strides, dv_strides, nullptr, B, H, 0, d, dtype_enum, causal, scale, hip_stream, variant);
    fa2_call_packed(c, l_head_stride, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, total_q, total_k, window_left, window_right);
    c.gqa = true; c.H_kv = H_kv;
    c.has_dv = true; c.d_v = d_v;
    return bwd(c);
}

}  // extern "C"
