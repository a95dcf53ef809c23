// Shared declarations of the gfx950 FA-2 backward kernels (internal; the public ABI is include/fa2_bwd.h).
#pragma once
#include "fa2_common.h"

#include "../../include/fa2_bwd.h"

// One backward problem, as handed over by fa2_bwd().  Strides in elements (src/flash_attention_torch.py:110-121).
struct Fa2BwdProblem {
    const void *Q, *K, *V, *O, *dO, *L;
    void *dQ, *dK, *dV, *D;
    int64_t qs[4], ks[4], vs[4], os[4], dos[4], dqs[4], dks[4], dvs[4], ls[2];
    int32_t B, H, N, d;
    int32_t dtype, causal;
    float scale;
    hipStream_t stream;
    int32_t wl, wr;  // local-attention window (fa2_bwd_window), normalised as in Fa2Problem
    // Variable-length (packed) problems (fa2_bwd_varlen), as in Fa2Problem: strides {0, head, token, dim}, ls = {0, head stride of
    // L}, raw window sides; D is the scratch of 2 * H * total_q accumulators ([2][H][total_q]).
    const int32_t *cu_q, *cu_k;
    int32_t max_q, max_k, total_q, total_k;
    int32_t dv;  // fa2_bwd_varlen_dv: the last axis of V, O, dO, dV (Q, K, dQ, dK keep d); 0 in every other call
};

// The six fa2_bwd_launch_generic* are all in fa2_bwd_generic.hip (the attention form is a parameter of its kernel templates); the
// matrix kernels' forms are a translation unit each.
int fa2_bwd_launch_generic(const Fa2BwdProblem &p);
int fa2_bwd_launch_mfma16(const Fa2BwdProblem &p);
int fa2_bwd_launch_generic_window(const Fa2BwdProblem &p);
int fa2_bwd_launch_mfma16_window(const Fa2BwdProblem &p);
int fa2_bwd_launch_generic_varlen(const Fa2BwdProblem &p);
int fa2_bwd_launch_mfma16_varlen(const Fa2BwdProblem &p);
// Grouped-query attention (fa2_bwd_gqa, fa2_bwd_varlen_gqa): K, V, dK, dV have p.H / gqa heads; dK / dV summed over each group in
// the kernel (a dense problem without a window runs the windowed form as the full band)
int fa2_bwd_launch_generic_window_gqa(const Fa2BwdProblem &p, int gqa);
int fa2_bwd_launch_mfma16_window_gqa(const Fa2BwdProblem &p, int gqa);
int fa2_bwd_launch_generic_varlen_gqa(const Fa2BwdProblem &p, int gqa);
int fa2_bwd_launch_mfma16_varlen_gqa(const Fa2BwdProblem &p, int gqa);
bool fa2_bwd_mfma16_supports(const Fa2BwdProblem &p);
// A value head size of its own (fa2_bwd_varlen_dv, p.dv != p.d): the varlen GQA VALU form over any (d, d_v), and the matrix kernel
// at d 192 / d_v 128 (fa2_bwd_mfma16dv.hip)
int fa2_bwd_launch_generic_varlen_dv(const Fa2BwdProblem &p, int gqa);
int fa2_bwd_launch_mfma16dv(const Fa2BwdProblem &p, int gqa);
bool fa2_bwd_mfma16dv_supports(const Fa2BwdProblem &p);
int fa2_bwd_launch_mfma32(const Fa2BwdProblem &p);
bool fa2_bwd_mfma32_supports(const Fa2BwdProblem &p);
