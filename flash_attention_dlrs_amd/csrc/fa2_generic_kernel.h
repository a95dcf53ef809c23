// fa2_generic_kernel.h -- the catch-all FA-2 forward kernel for gfx950 (launched from fa2_generic.hip).
//
// Covers everything the reference's host glue can hand to its Triton kernel
// (src/flash_attention_torch.py:24-47): every dtype of convert_triton_dtype (:7-18) plus bf16 / e4m3,
// arbitrary element strides on all four axes (src/flash_attention_kernels.py:45-79), any d in
// [1, 512] (the reference pads to a power of two on the host, torch.py:38), and -- beyond the reference, whose tiles need
// N % 16 == 0 (src/autotune_configs.py:184-187) -- any N >= 1.  It is the fallback behind the MFMA
// kernels (fa2_mfma16.hip, fa2_mfma32.hip), not the fast path: contractions run on the VALU.
//
// Arithmetic = the reference's, statement for statement (kernels.py:84-108): fp32 state (m, l, O),
// S = dot * log2e, exp2-domain online softmax, P rounded to the I/O dtype (RTNE) before P@V, O / l
// and L = m + log2 l rounded to the I/O dtype on store.  (float64 is carried in double: the
// reference cannot run that dtype at all, see oracle/fa2_oracle.c.)
//
// Work split: grid (ceil(N/16), B, H) -- axis order of kernels.py:38-40.  A 256-thread workgroup
// owns 16 query rows, 4 per wave.  Per 64-key tile: lane = key for the scores (one K row per lane,
// Q rows broadcast from LDS), wave shuffle reduction for the row max, then lane = output column
// for P@V with P broadcast from LDS.
//
// One kernel template serves every attention form: the form is the template parameter F, a set of the bits below, and each
// form's statements stand in an `if constexpr` branch of their own (merging branches into shared expressions costs registers:
// keep them apart).  F = 0 is the plain kernel.  The launchers in fa2_generic.hip name the six sets that exist.
//
// The 120 instantiations compile in two translation units, split by element type so that neither is the longest compile of the
// build: fa2_generic.hip (f32, f16, bf16) and fa2_generic_f64f8.hip (f64 and the two fp8 types, behind launch_f64_f8).
#pragma once
#include <math.h>

#include "fa2_common.h"
#include "fa2_elem.h"

namespace fa2_generic {

// kWindow: local attention -- key j visible to query i iff i - wl <= j <= i + wr.
// kVarlen (with kWindow): the variable-length form -- grid (ceil(max_q / 16), B, H), each workgroup reads its sequence's offsets and
// runs the windowed loop with the sequence's own query and key extents and the bottom-right shifted band (fa2_varlen_band); a row
// without a visible key gets O = 0, L = +inf.
// kGqa (with kWindow): grouped-query attention -- K and V have H / gqa heads and query head h reads KV head h / gqa.
// kDv (with kVarlen and kGqa): a value head size of its own (fa2_fwd_varlen_dv at d_v != d) -- the score loop runs over d, the
// output columns per lane come from d_v, LDS holds the Q tile at d.
// (the bits themselves: fa2_common.h)

constexpr int kRowsPerWave = 4;
constexpr int kWaves = 4;
constexpr int kBr = kRowsPerWave * kWaves;  // 16 = the reference's smallest B_r
constexpr int kBc = 64;                     // one key per lane

struct GenericArgs {  // fields a form does not use are 0
    const void *Q, *K, *V;
    void *O, *L;
    int64_t qs[4], ks[4], vs[4], os[4], ls[2];
    int N, d, causal;
    // kWindow: window sides, normalised to [0, N - 1] (fa2_window_normalise), causal is 0
    // kVarlen: raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    int wl, wr;
    const int32_t *cu_q, *cu_k;  // kVarlen
    int max_q, max_k, total_q, total_k;
    int gqa;  // kGqa: query heads per KV head
    int dv;   // kDv: columns of V and O
    double c_log2e;  // scale * log2(e); rounded to float for the fp32 dtypes (kernels.py:92)
};

// DPL = output columns per lane = ceil(d / 64) (kDv: ceil(d_v / 64)).
template <class E, int DPL, int F>
__global__ __launch_bounds__(kWaves * 64) void fa2_fwd_generic_kernel(const GenericArgs a) {
    using A = typename E::acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    A *q_lds = (A *)smem_raw;                           // [kBr][d]
    A *p_lds = q_lds + (size_t)kBr * a.d;               // [kWaves][kRowsPerWave][kBc]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x, b = blockIdx.y, h = blockIdx.z;  // kernels.py:38-40
    // N = the sequence's queries, NK its keys
    int qst = 0, N = a.N, kst = 0, NK = a.N;
    if constexpr (F & kVarlen) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, qst, N);
        fa2_varlen_seq(a.cu_k, b, a.total_k, a.max_k, kst, NK);
        if (i * kBr >= N) return;  // (whole workgroup, before any barrier)
    }
    const int d = a.d;
    const int dv = F & kDv ? a.dv : d;  // V's and O's columns
    const int hk = F & kGqa ? h / a.gqa : h;
    // kVarlen: bases in 64 bits from the sequence starts (token stride in qs[2], ...)
    const int64_t q_off = F & kVarlen ? (int64_t)qst * a.qs[2] + h * a.qs[1] : b * a.qs[0] + h * a.qs[1];
    const int64_t k_off = F & kVarlen ? (int64_t)kst * a.ks[2] + hk * a.ks[1] : b * a.ks[0] + hk * a.ks[1];
    const int64_t v_off = F & kVarlen ? (int64_t)kst * a.vs[2] + hk * a.vs[1] : b * a.vs[0] + hk * a.vs[1];
    const int64_t o_off = F & kVarlen ? (int64_t)qst * a.os[2] + h * a.os[1] : b * a.os[0] + h * a.os[1];

    // Q tile -> LDS (rows past N are clamped; their results are never stored).
    for (int idx = tid; idx < kBr * d; idx += kWaves * 64) {
        const int r = idx / d, x = idx - r * d;
        int row = i * kBr + r;
        row = row < N ? row : N - 1;
        q_lds[idx] = E::load(a.Q, q_off + (int64_t)row * a.qs[2] + (int64_t)x * a.qs[3]);
    }
    __syncthreads();

    const A c = sizeof(A) == 8 ? (A)a.c_log2e : (A)(float)a.c_log2e;
    const int row0 = i * kBr + wave * kRowsPerWave;
    A m[kRowsPerWave], lsum[kRowsPerWave], o[kRowsPerWave][DPL];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        m[r] = -INFINITY;
        lsum[r] = 0;
#pragma unroll
        for (int cc = 0; cc < DPL; ++cc) o[r][cc] = 0;
    }

    // Same trip count for every wave of the workgroup (barriers inside).
    int wl = a.wl, wr = a.wr;
    if constexpr (F & kVarlen) fa2_varlen_band(N, NK, a.causal, a.wl, a.wr, wl, wr);
    int kbeg = 0, kend = N;
    if constexpr (F & kWindow) {  // the keys of its 16 rows, [i kBr - wl, i kBr + 15 + wr]
        kbeg = i * kBr - wl > 0 ? i * kBr - wl : 0;
        kend = i * kBr + kBr + wr < NK ? i * kBr + kBr + wr : NK;
    } else if (a.causal) {
        const int lim = i * kBr + kBr;
        kend = lim < N ? lim : N;
    }
    A *p_w = p_lds + (size_t)wave * kRowsPerWave * kBc;

    for (int kt = kbeg; kt < kend; kt += kBc) {
        const int key = kt + lane;
        const bool valid = key < NK;
        A dot[kRowsPerWave];
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) dot[r] = 0;
        if (valid) {
            const int64_t kb = k_off + (int64_t)key * a.ks[2];
            for (int x = 0; x < d; ++x) {
                const A kx = E::load(a.K, kb + (int64_t)x * a.ks[3]);
#pragma unroll
                for (int r = 0; r < kRowsPerWave; ++r)
                    dot[r] += q_lds[(wave * kRowsPerWave + r) * d + x] * kx;
            }
        }
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            A s = dot[r] * c;  // kernels.py:92
            A m_new, p, coeff;
            if constexpr (F & kWindow) {
                if (!valid || key < row0 + r - wl || key > row0 + r + wr) s = -INFINITY;
                const A mx = wave_max(s);
                m_new = m[r] > mx ? m[r] : mx;
                // a row may meet whole tiles before its band starts: while its maximum is -inf, P and the rescale factor are 0
                // (not exp2(-inf + inf))
                const A m_use = m_new == -INFINITY ? (A)0 : m_new;
                p = exp2_acc<A>(s - m_use);
                coeff = exp2_acc<A>(m[r] - m_use);
            } else {
                if (!valid || (a.causal && key > row0 + r)) s = -INFINITY;
                const A mx = wave_max(s);
                m_new = m[r] > mx ? m[r] : mx;           // :93
                p = exp2_acc<A>(s - m_new);              // :94
                coeff = exp2_acc<A>(m[r] - m_new);       // :95
            }
            lsum[r] = coeff * lsum[r] + p;                   // :96 (per-lane partial of the row sum)
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) o[r][cc] *= coeff;  // :97
            m[r] = m_new;                                    // :99
            p_w[r * kBc + lane] = E::round(p);               // :98 cast(P)
        }
        __syncthreads();
        const int kmax = (NK - kt) < kBc ? (NK - kt) : kBc;
        for (int kk = 0; kk < kmax; ++kk) {
            const int64_t vb = v_off + (int64_t)(kt + kk) * a.vs[2];
            A pr[kRowsPerWave];
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) pr[r] = p_w[r * kBc + kk];
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) {
                    const A v = E::load(a.V, vb + (int64_t)x * a.vs[3]);
#pragma unroll
                    for (int r = 0; r < kRowsPerWave; ++r) o[r][cc] += pr[r] * v;  // :98
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int row = row0 + r;
        const A l = wave_sum(lsum[r]);
        if (row < N) {
            if constexpr (F & kVarlen) {
                // a row without a visible key: O = 0 and L = +inf (the backward then recomputes P = 0)
#pragma unroll
                for (int cc = 0; cc < DPL; ++cc) {
                    const int x = lane + 64 * cc;
                    if (x < dv)
                        E::store(a.O, o_off + (int64_t)row * a.os[2] + (int64_t)x * a.os[3], l > 0 ? o[r][cc] / l : (A)0);
                }
                if (lane == 0)
                    E::store(a.L, h * a.ls[1] + qst + row, l > 0 ? m[r] + log2_acc<A>(l) : (A)INFINITY);
            } else {
#pragma unroll
                for (int cc = 0; cc < DPL; ++cc) {
                    const int x = lane + 64 * cc;
                    if (x < dv)
                        E::store(a.O, o_off + (int64_t)row * a.os[2] + (int64_t)x * a.os[3], o[r][cc] / l);  // :105,:107
                }
                if (lane == 0)
                    E::store(a.L, b * a.ls[0] + h * a.ls[1] + row, m[r] + log2_acc<A>(l));  // :106,:108
            }
        }
    }
}

template <class E, int F> int launch_e(const Fa2Problem &p, const GenericArgs &a) {
    const dim3 grid(((F & kVarlen ? p.max_q : p.N) + kBr - 1) / kBr, p.B, p.H), block(kWaves * 64);
    const size_t smem = sizeof(typename E::acc_t) * ((size_t)kBr * p.d + (size_t)kWaves * kRowsPerWave * kBc);
    // output columns per lane: ceil(d / 64) rounded up to the next instantiation (columns >= d are skipped in the kernel)
    const int dpl = ((F & kDv ? p.dv : p.d) + 63) / 64;
    if (dpl <= 1) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 1, F>), grid, block, smem, p.stream, a);
    else if (dpl <= 2) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 2, F>), grid, block, smem, p.stream, a);
    else if (dpl <= 4) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 4, F>), grid, block, smem, p.stream, a);
    else if (dpl <= 8) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 8, F>), grid, block, smem, p.stream, a);
    else {
        fa2_set_error("generic kernel: d=%d not in [1, 512]", p.d);
        return FA2_ERR_UNSUPPORTED;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("generic kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

// f64 and the two fp8 types of form F: defined and instantiated in fa2_generic_f64f8.hip
template <int F> int launch_f64_f8(const Fa2Problem &p, const GenericArgs &a);

}  // namespace fa2_generic
