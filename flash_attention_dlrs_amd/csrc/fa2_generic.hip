// fa2_generic.hip -- the catch-all FA-2 forward kernel for gfx950.
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
#include <math.h>

#include "fa2_common.h"
#include "fa2_elem.h"

// FA2_GENERIC_WINDOW (fa2_generic_w.hip): the local-attention form -- key j visible to query i iff i - wl <= j <= i + wr -- under
// its own kernel name, compiled in a translation unit of its own; without the macro this file is the plain kernel, unchanged.
// FA2_GENERIC_VARLEN (fa2_generic_v.hip, on top of FA2_GENERIC_WINDOW): the variable-length form -- grid (ceil(max_q / 16), B, H),
// each workgroup reads its sequence's offsets and runs the windowed loop with the sequence's own query and key extents and the
// bottom-right shifted band (fa2_varlen_band); a row without a visible key gets O = 0, L = +inf.
// FA2_GENERIC_GQA (fa2_generic_wg.hip, fa2_generic_vg.hip, on top of the windowed or varlen form): grouped-query attention -- K and V
// have H / gqa heads and query head h reads KV head h / gqa.
// FA2_GENERIC_DV (fa2_generic_vgd.hip, on top of the varlen GQA form): a value head size of its own -- the score loop runs over d,
// the output columns per lane come from d_v, LDS holds the Q tile at d -- under its own kernel name (fa2_fwd_varlen_dv at d_v != d).
#if defined(FA2_GENERIC_DV)
#define fa2_fwd_generic_kernel fa2_fwd_generic_varlen_dv_kernel
#elif defined(FA2_GENERIC_GQA) && defined(FA2_GENERIC_VARLEN)
#define fa2_fwd_generic_kernel fa2_fwd_generic_varlen_gqa_kernel
#elif defined(FA2_GENERIC_GQA)
#define fa2_fwd_generic_kernel fa2_fwd_generic_window_gqa_kernel
#elif defined(FA2_GENERIC_VARLEN)
#define fa2_fwd_generic_kernel fa2_fwd_generic_varlen_kernel
#elif defined(FA2_GENERIC_WINDOW)
#define fa2_fwd_generic_kernel fa2_fwd_generic_window_kernel
#endif

namespace {

constexpr int kRowsPerWave = 4;
constexpr int kWaves = 4;
constexpr int kBr = kRowsPerWave * kWaves;  // 16 = the reference's smallest B_r
constexpr int kBc = 64;                     // one key per lane

struct GenericArgs {
    const void *Q, *K, *V;
    void *O, *L;
    int64_t qs[4], ks[4], vs[4], os[4], ls[2];
#if defined(FA2_GENERIC_VARLEN)
    int N, d, causal;
    int wl, wr;  // raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    const int32_t *cu_q, *cu_k;
    int max_q, max_k, total_q, total_k;
#elif defined(FA2_GENERIC_WINDOW)
    int N, d, causal;
    int wl, wr;  // window sides, normalised to [0, N - 1] (fa2_window_normalise); causal is 0
#else
    int N, d, causal;
#endif
#ifdef FA2_GENERIC_GQA
    int gqa;  // query heads per KV head
#endif
#ifdef FA2_GENERIC_DV
    int dv;  // columns of V and O
#endif
    double c_log2e;  // scale * log2(e); rounded to float for the fp32 dtypes (kernels.py:92)
};

// DPL = output columns per lane = ceil(d / 64) (FA2_GENERIC_DV: ceil(d_v / 64)).
template <class E, int DPL>
__global__ __launch_bounds__(kWaves * 64) void fa2_fwd_generic_kernel(const GenericArgs a) {
    using A = typename E::acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    A *q_lds = (A *)smem_raw;                           // [kBr][d]
    A *p_lds = q_lds + (size_t)kBr * a.d;               // [kWaves][kRowsPerWave][kBc]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x, b = blockIdx.y, h = blockIdx.z;  // kernels.py:38-40
#ifdef FA2_GENERIC_VARLEN
    // N = the sequence's queries, NK its keys; bases in 64 bits from the sequence starts (token stride in qs[2], ...)
    int qst, N, kst, NK;
    fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, qst, N);
    fa2_varlen_seq(a.cu_k, b, a.total_k, a.max_k, kst, NK);
    if (i * kBr >= N) return;  // (whole workgroup, before any barrier)
    const int d = a.d;
#ifdef FA2_GENERIC_GQA
    const int hk = h / a.gqa;
    const int64_t q_off = (int64_t)qst * a.qs[2] + h * a.qs[1];
    const int64_t k_off = (int64_t)kst * a.ks[2] + hk * a.ks[1];
    const int64_t v_off = (int64_t)kst * a.vs[2] + hk * a.vs[1];
    const int64_t o_off = (int64_t)qst * a.os[2] + h * a.os[1];
#else
    const int64_t q_off = (int64_t)qst * a.qs[2] + h * a.qs[1];
    const int64_t k_off = (int64_t)kst * a.ks[2] + h * a.ks[1];
    const int64_t v_off = (int64_t)kst * a.vs[2] + h * a.vs[1];
    const int64_t o_off = (int64_t)qst * a.os[2] + h * a.os[1];
#endif
#elif defined(FA2_GENERIC_GQA)
    const int N = a.N, d = a.d;
    const int NK = N;
    const int hk = h / a.gqa;
    const int64_t q_off = b * a.qs[0] + h * a.qs[1];
    const int64_t k_off = b * a.ks[0] + hk * a.ks[1];
    const int64_t v_off = b * a.vs[0] + hk * a.vs[1];
    const int64_t o_off = b * a.os[0] + h * a.os[1];
#else
    const int N = a.N, d = a.d;
    const int NK = N;
    const char *Qb = (const char *)a.Q;
    const int64_t q_off = b * a.qs[0] + h * a.qs[1];
    const int64_t k_off = b * a.ks[0] + h * a.ks[1];
    const int64_t v_off = b * a.vs[0] + h * a.vs[1];
    const int64_t o_off = b * a.os[0] + h * a.os[1];
    (void)Qb;
#endif
#ifdef FA2_GENERIC_DV
    const int dv = a.dv;
#else
    const int dv = d;  // V's and O's columns
#endif

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

#ifdef FA2_GENERIC_WINDOW
    // Same trip count for every wave of the workgroup (barriers inside): the keys of its 16 rows, [i kBr - wl, i kBr + 15 + wr]
#ifdef FA2_GENERIC_VARLEN
    int wl, wr;
    fa2_varlen_band(N, NK, a.causal, a.wl, a.wr, wl, wr);
#else
    const int wl = a.wl, wr = a.wr;
#endif
    const int kbeg = i * kBr - wl > 0 ? i * kBr - wl : 0;
    const int kend = i * kBr + kBr + wr < NK ? i * kBr + kBr + wr : NK;
    A *p_w = p_lds + (size_t)wave * kRowsPerWave * kBc;

    for (int kt = kbeg; kt < kend; kt += kBc) {
#else
    // Same trip count for every wave of the workgroup (barriers inside).
    int kend = N;
    if (a.causal) {
        const int lim = i * kBr + kBr;
        kend = lim < N ? lim : N;
    }
    A *p_w = p_lds + (size_t)wave * kRowsPerWave * kBc;

    for (int kt = 0; kt < kend; kt += kBc) {
#endif
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
#ifdef FA2_GENERIC_WINDOW
            if (!valid || key < row0 + r - wl || key > row0 + r + wr) s = -INFINITY;
            const A mx = wave_max(s);
            const A m_new = m[r] > mx ? m[r] : mx;
            // a row may meet whole tiles before its band starts: while its maximum is -inf, P and the rescale factor are 0
            // (not exp2(-inf + inf))
            const A m_use = m_new == -INFINITY ? (A)0 : m_new;
            const A p = exp2_acc<A>(s - m_use);
            const A coeff = exp2_acc<A>(m[r] - m_use);
#else
            if (!valid || (a.causal && key > row0 + r)) s = -INFINITY;
            const A mx = wave_max(s);
            const A m_new = m[r] > mx ? m[r] : mx;           // :93
            const A p = exp2_acc<A>(s - m_new);              // :94
            const A coeff = exp2_acc<A>(m[r] - m_new);       // :95
#endif
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
#ifdef FA2_GENERIC_VARLEN
            // a row without a visible key: O = 0 and L = +inf (the backward then recomputes P = 0)
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv)
                    E::store(a.O, o_off + (int64_t)row * a.os[2] + (int64_t)x * a.os[3], l > 0 ? o[r][cc] / l : (A)0);
            }
            if (lane == 0)
                E::store(a.L, h * a.ls[1] + qst + row, l > 0 ? m[r] + log2_acc<A>(l) : (A)INFINITY);
#else
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv)
                    E::store(a.O, o_off + (int64_t)row * a.os[2] + (int64_t)x * a.os[3], o[r][cc] / l);  // :105,:107
            }
            if (lane == 0)
                E::store(a.L, b * a.ls[0] + h * a.ls[1] + row, m[r] + log2_acc<A>(l));  // :106,:108
#endif
        }
    }
}

template <class E> int launch_e(const Fa2Problem &p, const GenericArgs &a) {
#ifdef FA2_GENERIC_VARLEN
    const dim3 grid((p.max_q + kBr - 1) / kBr, p.B, p.H), block(kWaves * 64);
#else
    const dim3 grid((p.N + kBr - 1) / kBr, p.B, p.H), block(kWaves * 64);
#endif
    const size_t smem = sizeof(typename E::acc_t) * ((size_t)kBr * p.d + (size_t)kWaves * kRowsPerWave * kBc);
    // output columns per lane: ceil(d / 64) rounded up to the next instantiation (columns >= d are skipped in the kernel)
#ifdef FA2_GENERIC_DV
    const int dpl = (p.dv + 63) / 64;
#else
    const int dpl = (p.d + 63) / 64;
#endif
    if (dpl <= 1) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 1>), grid, block, smem, p.stream, a);
    else if (dpl <= 2) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 2>), grid, block, smem, p.stream, a);
    else if (dpl <= 4) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 4>), grid, block, smem, p.stream, a);
    else if (dpl <= 8) hipLaunchKernelGGL((fa2_fwd_generic_kernel<E, 8>), grid, block, smem, p.stream, a);
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

}  // namespace

#if defined(FA2_GENERIC_DV)
int fa2_launch_generic_varlen_dv(const Fa2Problem &p, int gqa) {
#elif defined(FA2_GENERIC_GQA) && defined(FA2_GENERIC_VARLEN)
int fa2_launch_generic_varlen_gqa(const Fa2Problem &p, int gqa) {
#elif defined(FA2_GENERIC_GQA)
int fa2_launch_generic_window_gqa(const Fa2Problem &p, int gqa) {
#elif defined(FA2_GENERIC_VARLEN)
int fa2_launch_generic_varlen(const Fa2Problem &p) {
#elif defined(FA2_GENERIC_WINDOW)
int fa2_launch_generic_window(const Fa2Problem &p) {
#else
int fa2_launch_generic(const Fa2Problem &p) {
#endif
    if (p.B > 65535 || p.H > 65535) {
        fa2_set_error("generic kernel: B and H must be <= 65535");
        return FA2_ERR_BAD_ARG;
    }
    GenericArgs a;
    a.Q = p.Q; a.K = p.K; a.V = p.V; a.O = p.O; a.L = p.L;
    for (int k = 0; k < 4; ++k) { a.qs[k] = p.qs[k]; a.ks[k] = p.ks[k]; a.vs[k] = p.vs[k]; a.os[k] = p.os[k]; }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
#if defined(FA2_GENERIC_VARLEN)
    a.N = p.N; a.d = p.d; a.causal = p.causal; a.wl = p.wl; a.wr = p.wr;
    a.cu_q = p.cu_q; a.cu_k = p.cu_k; a.max_q = p.max_q; a.max_k = p.max_k; a.total_q = p.total_q; a.total_k = p.total_k;
    if (p.max_q == 0) return FA2_OK;  // no query rows anywhere
#elif defined(FA2_GENERIC_WINDOW)
    a.N = p.N; a.d = p.d; a.causal = 0; a.wl = p.wl; a.wr = p.wr;
#else
    a.N = p.N; a.d = p.d; a.causal = p.causal;
#endif
    a.c_log2e = (double)p.scale * FA2_LOG2E;
#ifdef FA2_GENERIC_GQA
    a.gqa = gqa;
#endif
#ifdef FA2_GENERIC_DV
    a.dv = p.dv;
#endif
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32>(p, a);
    case FA2_DTYPE_F16: return launch_e<ElemF16>(p, a);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16>(p, a);
#ifndef FA2_GENERIC_VARLEN  // (fp8 has no varlen form: no backward, and e4m3fn cannot hold L = +inf)
    case FA2_DTYPE_F8E5M2: return launch_e<ElemF8E5M2>(p, a);
    case FA2_DTYPE_F8E4M3: return launch_e<ElemF8E4M3>(p, a);
#endif
    case FA2_DTYPE_F64: return launch_e<ElemF64>(p, a);
    default: fa2_set_error("unknown dtype enum %d", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}
