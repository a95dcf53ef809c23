// fa2_generic.hip -- the launchers of the catch-all FA-2 forward kernel (fa2_generic_kernel.h), one per attention form, and its
// f32 / f16 / bf16 instantiations; the other element types compile in fa2_generic_f64f8.hip.
#include "fa2_generic_kernel.h"

using namespace fa2_generic;

namespace {

template <int F> int launch_form(const Fa2Problem &p, int gqa) {
    if (p.B > 65535 || p.H > 65535) {
        fa2_set_error("generic kernel: B and H must be <= 65535");
        return FA2_ERR_BAD_ARG;
    }
    GenericArgs a = {};
    a.Q = p.Q; a.K = p.K; a.V = p.V; a.O = p.O; a.L = p.L;
    for (int k = 0; k < 4; ++k) { a.qs[k] = p.qs[k]; a.ks[k] = p.ks[k]; a.vs[k] = p.vs[k]; a.os[k] = p.os[k]; }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.N = p.N; a.d = p.d;
    a.causal = (F & (kWindow | kVarlen)) == kWindow ? 0 : p.causal;  // (a dense window arrives normalised: causal is in its sides)
    if constexpr (F & kWindow) { a.wl = p.wl; a.wr = p.wr; }
    if constexpr (F & kVarlen) {
        a.cu_q = p.cu_q; a.cu_k = p.cu_k; a.max_q = p.max_q; a.max_k = p.max_k; a.total_q = p.total_q; a.total_k = p.total_k;
        if (p.max_q == 0) return FA2_OK;  // no query rows anywhere
    }
    if constexpr (F & kGqa) a.gqa = gqa;
    if constexpr (F & kDv) a.dv = p.dv;
    a.c_log2e = (double)p.scale * FA2_LOG2E;
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32, F>(p, a);
    case FA2_DTYPE_F16: return launch_e<ElemF16, F>(p, a);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16, F>(p, a);
    default: return launch_f64_f8<F>(p, a);
    }
}

}  // namespace

int fa2_launch_generic(const Fa2Problem &p) { return launch_form<0>(p, 1); }
int fa2_launch_generic_window(const Fa2Problem &p) { return launch_form<kWindow>(p, 1); }
int fa2_launch_generic_varlen(const Fa2Problem &p) { return launch_form<kWindow | kVarlen>(p, 1); }
int fa2_launch_generic_window_gqa(const Fa2Problem &p, int gqa) { return launch_form<kWindow | kGqa>(p, gqa); }
int fa2_launch_generic_varlen_gqa(const Fa2Problem &p, int gqa) { return launch_form<kWindow | kVarlen | kGqa>(p, gqa); }
int fa2_launch_generic_varlen_dv(const Fa2Problem &p, int gqa) { return launch_form<kWindow | kVarlen | kGqa | kDv>(p, gqa); }
