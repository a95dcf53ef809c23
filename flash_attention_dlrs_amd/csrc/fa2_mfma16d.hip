// fa2_mfma16d.hip -- the launchers of the LDS-DMA forward kernel (fa2_mfma16d_kernel.h, variant "mfma16d"), one per attention form,
// and its bf16 instantiations; the f16 ones compile in fa2_mfma16d_f16.hip.
#include "fa2_mfma16d_kernel.h"

using namespace fa2_mfma16d;

namespace {

template <int F> int launch_form(const Fa2Problem &pv, int waves, int gqa) {
    Fa2Problem p = pv;
    if constexpr (F & kVarlen) p.causal = 0;  // the causal mask is in the band (fa2_varlen_band): one tile per workgroup, no tile pairs
    // 32-bit buffer offsets span one sequence: kVarlen is judged on max_seqlen x row stride, not on the packed total
    const int nk = F & kVarlen ? p.max_k : p.N;
    const bool fits32 = (int64_t)(nk + 512) * p.ks[2] * 2 < (1LL << 31) && (int64_t)(nk + 512) * p.vs[2] * 2 < (1LL << 31);
    if (!fa2_mfma16_supports(p) || !fits32) {
        fa2_set_error("mfma16d kernel: needs f16/bf16, d in {64,128}, unit d-stride, 16-byte aligned rows, scale > 0, "
                      "N * row stride < 2 GiB");
        return FA2_ERR_UNSUPPORTED;
    }
    DmaArgs a = {};
    a.Q = (const char *)p.Q; a.K = (const char *)p.K; a.V = (const char *)p.V;
    a.O = (char *)p.O; a.L = (char *)p.L;
    for (int k = 0; k < 3; ++k) {
        a.qs[k] = p.qs[k] * 2; a.ks[k] = p.ks[k] * 2; a.vs[k] = p.vs[k] * 2; a.os[k] = p.os[k] * 2;
    }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.B = p.B; a.H = p.H; a.N = p.N;
    a.c_log2e = (float)((double)p.scale * FA2_LOG2E);
    a.group = 1;
    a.flags = fa2_env_int("FA2_FLAGS", 0);
    if constexpr (F & kWindow) { a.wl = p.wl; a.wr = p.wr; }
    if constexpr (F & kVarlen) {
        a.causal = pv.causal;
        a.cu_q = p.cu_q; a.cu_k = p.cu_k; a.max_q = p.max_q; a.max_k = p.max_k; a.total_q = p.total_q; a.total_k = p.total_k;
        if (p.max_q == 0) return FA2_OK;  // no query rows anywhere
    }
    if constexpr (F & kGqa) a.gqa = gqa;
    if (p.causal && ((p.B * p.H) & 7) == 0) {
        const int per_xcd = p.B * p.H / 8;
        int g = fa2_env_int("FA2_CAUSAL_GROUP", 2);
        g = g < 1 ? 1 : (g > per_xcd ? per_xcd : g);
        while (per_xcd % g) --g;
        a.group = g;
    }
    return p.dtype == FA2_DTYPE_BF16 ? launch_d<__bf16, F>(p, a, waves) : launch_f16<F>(p, a, waves);
}

}  // namespace

int fa2_launch_mfma16d(const Fa2Problem &p, int waves) { return launch_form<0>(p, waves, 1); }
int fa2_launch_mfma16d_window(const Fa2Problem &p, int waves) { return launch_form<kWindow>(p, waves, 1); }
int fa2_launch_mfma16d_varlen(const Fa2Problem &p, int waves) { return launch_form<kWindow | kVarlen>(p, waves, 1); }
int fa2_launch_mfma16d_window_gqa(const Fa2Problem &p, int waves, int gqa) { return launch_form<kWindow | kGqa>(p, waves, gqa); }
int fa2_launch_mfma16d_varlen_gqa(const Fa2Problem &p, int waves, int gqa) {
    return launch_form<kWindow | kVarlen | kGqa>(p, waves, gqa);
}
