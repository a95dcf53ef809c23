// fa2_host.h -- what the host paths of the training forward (fa2_api.hip) and backward (fa2_bwd_api.hip) share: the form a checked
// call runs in, and the checks both directions make with one message -- the window sides, the sizes of a packed call -- with the
// packed stride conversion.  Both files take the same three steps per entry point: fill a call struct (FwdCall / BwdCall), check
// it (check_fwd / check_bwd: every argument, in one order, yielding the problem and the form), run the form's table.
#pragma once
#include "fa2_common.h"

// The form a checked call runs in.  DENSE is plain or causal attention -- a window that removes nothing more included, and a GQA
// layout merged into an MHA problem -- and has each direction's full variant table; the other four have the small one (kForms).
enum { FA2_FORM_DENSE, FA2_FORM_WINDOW, FA2_FORM_VARLEN, FA2_FORM_WINDOW_GQA, FA2_FORM_VARLEN_GQA };
struct Fa2Form {
    int kind;
    int g;  // H / H_kv, 1 without GQA: the GQA launchers' group size
};

static inline int fa2_check_window_sides(int32_t wl, int32_t wr) {
    if (wl < -1 || wr < -1) {
        fa2_set_error("window sides must be >= -1 (-1 = unbounded), got window=(%d, %d)", wl, wr);
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

// The window of a dense call: the sides refused or normalised (fa2_window_normalise).  N < 1 is validate()'s to report, after this.
struct Fa2Window {
    int32_t causal, wl, wr, windowed;
};
static inline int fa2_window_of(int32_t N, int32_t causal, int32_t wl, int32_t wr, Fa2Window &w) {
    w = {causal ? 1 : 0, 0, 0, 0};
    if (N < 1) return fa2_check_window_sides(wl, wr);
    return fa2_window_normalise(N, causal, wl, wr, &w.causal, &w.wl, &w.wr, &w.windowed);
}

// The first null of `n` pointers, by name; `who` ("varlen", "varlen backward") opens every message of a packed call.
static inline int fa2_check_nonnull(const char *who, const void *const *ptrs, const char *const *names, int n) {
    for (int t = 0; t < n; ++t)
        if (!ptrs[t]) {
            fa2_set_error("%s: null %s", who, names[t]);
            return FA2_ERR_BAD_ARG;
        }
    return FA2_OK;
}

// The sizes of a packed call (FwdCall / BwdCall), its offsets and its window sides.  The forward refuses H < 1 here (h_from_1), the
// backward leaves it to validate().
template <typename Call> int fa2_check_packed(const char *who, const Call &c, bool h_from_1) {
    if (!c.cu_seqlens_q || !c.cu_seqlens_k) {
        fa2_set_error("%s: null %s", who, !c.cu_seqlens_q ? "cu_seqlens_q" : "cu_seqlens_k");
        return FA2_ERR_BAD_ARG;
    }
    if (c.B < 1 || c.B > 65535) {
        fa2_set_error("%s: B (number of sequences) must be in [1, 65535] (got %d)", who, c.B);
        return FA2_ERR_BAD_ARG;
    }
    if (c.H > 65535 || (h_from_1 && c.H < 1)) {
        fa2_set_error(h_from_1 ? "%s: H must be in [1, 65535] (got %d)" : "%s: H must be <= 65535 (got %d)", who, c.H);
        return FA2_ERR_BAD_ARG;
    }
    if (c.max_seqlen_q < 0 || c.max_seqlen_k < 0 || c.max_seqlen_q > (1 << 28) || c.max_seqlen_k > (1 << 28)) {
        fa2_set_error("%s: max_seqlen_q and max_seqlen_k must be in [0, 2^28] (got %d, %d)", who, c.max_seqlen_q, c.max_seqlen_k);
        return FA2_ERR_BAD_ARG;
    }
    if (c.total_q < 0 || c.total_k < 0) {
        fa2_set_error("%s: total_q and total_k must be >= 0 (got %d, %d)", who, c.total_q, c.total_k);
        return FA2_ERR_BAD_ARG;
    }
    return fa2_check_window_sides(c.window_left, c.window_right);
}

// Packed strides {token, head, d} as a problem's four {0, head, token, d}.
static inline void fa2_packed_strides4(const int64_t s3[3], int64_t s4[4]) {
    s4[0] = 0; s4[1] = s3[1]; s4[2] = s3[0]; s4[3] = s3[2];
}

// The packed part of a checked call in its problem (Fa2Problem / Fa2BwdProblem): raw window sides, offsets, sizes, L's head stride,
// and N -- only for validate() and the support predicates -- the longest extent, at least 1.
template <typename Call, typename Problem> void fa2_set_packed(const Call &c, Problem &p) {
    const int32_t nmax = c.max_seqlen_q > c.max_seqlen_k ? c.max_seqlen_q : c.max_seqlen_k;
    p.N = nmax > 0 ? nmax : 1;
    p.ls[0] = 0; p.ls[1] = c.l_head_stride;
    p.wl = c.window_left; p.wr = c.window_right;
    p.cu_q = c.cu_seqlens_q; p.cu_k = c.cu_seqlens_k;
    p.max_q = c.max_seqlen_q; p.max_k = c.max_seqlen_k; p.total_q = c.total_q; p.total_k = c.total_k;
}

// The packed arguments of an entry point in its call (FwdCall / BwdCall).
template <typename Call>
void fa2_call_packed(Call &c, int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t max_seqlen_q,
                     int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t window_left, int32_t window_right) {
    c.packed = true;
    c.l_head_stride = l_head_stride; c.cu_seqlens_q = cu_seqlens_q; c.cu_seqlens_k = cu_seqlens_k;
    c.max_seqlen_q = max_seqlen_q; c.max_seqlen_k = max_seqlen_k; c.total_q = total_q; c.total_k = total_k;
    c.window_left = window_left; c.window_right = window_right;
}
