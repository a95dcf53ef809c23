// fa2_bwd_generic.hip -- catch-all FA-2 backward kernels for gfx950 (contractions on the VALU).
//
// Covers what the reference's backward glue can hand to its kernels (src/flash_attention_torch.py:86-158):
// fp64 / fp32 / fp16 (+ bf16), arbitrary element strides, d = 2^k in [16, 512], and any N >= 1.  It is the
// fallback behind fa2_bwd_mfma16.hip and the path of the reference's own fp32 gradcheck (src/test_torch.py).
//
// Arithmetic = the reference's (src/flash_attention_kernels.py):
//   D  = rowsum(dO * O)                               bwd_D_kernel :115-166  (kept in the accumulate type)
//   S  = Q K^T * log2e ; P = exp2(S - L)              bwd_kernel   :283-285
//   dV += cast(P)^T dO                                             :287
//   dP = dO V^T ; dS = P * (dP - D)                                :289-291
//   dK += cast(dS)^T Q ; dQ += cast(dS) K                          :293, :317
// with P and dS rounded to the I/O dtype (RTNE) before the second contractions as the reference's casts do, and
// every accumulation in fp32 (fp64 for the fp64 dtype) -- the reference accumulates dK/dV/dQ in the I/O dtype
// (out_dtype=..., rounding at every query / key block), which this does not imitate.
//
// Work split (no cross-workgroup sums, hence deterministic; include/fa2_bwd.h):
//   bwd_dkdv: one workgroup per block of TB keys, sweeping the query rows TB at a time  -> dK, dV
//   bwd_dq:   one workgroup per block of TB query rows, sweeping the keys TB at a time  -> dQ
// TB x TB (P, dS) pairs are one thread each; the TB x d outputs are spread over the 256 threads and live in LDS.
//
// One pair of kernel templates serves every attention form: the form is the template parameter F, a set of the bits below, and
// each form's statements stand in an `if constexpr` branch of their own (as in fa2_generic.hip).  F = 0 is the plain kernels.  The
// launchers at the end of the file name the six sets that exist.
#include "fa2_bwd_common.h"
#include "fa2_elem.h"

namespace {

// kWindow: local attention -- key j visible to query i iff i - wl <= j <= i + wr.
// kVarlen (with kWindow): the variable-length form -- MODE 0 owns one sequence's key block and sweeps only that sequence's queries,
// MODE 1 the reverse; per-sequence extents, bottom-right shifted band (fa2_varlen_band).  D and the row statistic are laid out
// [H][total_q].  A row without a visible key (L = +inf) has P = 0: its dQ is 0 and its statistic stays +inf (not inf + log2(0)).
// kGqa (with kWindow): grouped-query attention -- K, V, dK, dV have H / gqa heads.  MODE 1 (grid z = query head h) reads KV head
// h / gqa; MODE 0 (grid z = KV head k) sweeps the queries of its g query heads k * gqa ... k * gqa + gqa - 1 in turn into the same
// accumulators and stores once: the group sum of dK / dV without atomics, in a fixed order.
// kDv (with kVarlen and kGqa): a value head size of its own (fa2_bwd_varlen_dv) -- V, O, dO and dV have a.dv columns: the second
// owned / swept operand, the dV accumulator, dP = dO V^T and D = rowsum(dO * O) run over dv, everything on the Q / K / dQ / dK
// side over d.
// (the bits themselves: fa2_common.h)

struct GArgs {  // fields a form does not use are 0
    const void *Q, *K, *V, *O, *dO, *L;
    void *dQ, *dK, *dV, *D;
    int64_t qs[4], ks[4], vs[4], os[4], dos[4], dqs[4], dks[4], dvs[4], ls[2];
    int H, N, d, causal, TB;
    // kWindow: window sides, normalised to [0, N - 1] (fa2_window_normalise), causal is 0
    // kVarlen: raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    int wl, wr;
    const int32_t *cu_q, *cu_k;  // kVarlen
    int max_q, max_k, total_q, total_k;
    double c_log2e, scale;
    int gqa;  // query heads per KV head (1 without kGqa)
    int dv;   // kDv: columns of V, O, dO, dV
};

// D[b, h, n] = sum_x O[b, h, n, x] * dO[b, h, n, x]   (kernels.py:115-166)
template <typename E, int F> __global__ __launch_bounds__(256) void bwd_D_kernel(const GArgs a, long long rows) {
    using A = typename E::acc_t;
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int64_t o0, g0;
    if constexpr (F & kVarlen) {
        // D[h][token], every packed token (rows = H * total_q)
        const int n = (int)(r % a.total_q), h = (int)(r / a.total_q);
        o0 = h * a.os[1] + (int64_t)n * a.os[2];
        g0 = h * a.dos[1] + (int64_t)n * a.dos[2];
    } else {
        const int n = (int)(r % a.N);
        const long long bh = r / a.N;
        const int h = (int)(bh % a.H), b = (int)(bh / a.H);
        o0 = b * a.os[0] + h * a.os[1] + n * a.os[2];
        g0 = b * a.dos[0] + h * a.dos[1] + n * a.dos[2];
    }
    const int dv = F & kDv ? a.dv : a.d;
    A s = 0;
    for (int x = 0; x < dv; ++x) s += E::load(a.O, o0 + x * a.os[3]) * E::load(a.dO, g0 + x * a.dos[3]);
    ((A *)a.D)[r] = s;
}

// MODE 0: key-block owner (dK, dV).  MODE 1: query-block owner (dQ).
template <typename E, int MODE, int F> __global__ __launch_bounds__(256) void bwd_main_kernel(const GArgs a) {
    using A = typename E::acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int TB = a.TB, d = a.d, ld = d + 1, tid = threadIdx.x;
    const int dv = F & kDv ? a.dv : d, ldv = dv + 1;  // the second operands and dV: dv columns
    A *own0 = (A *)smem_raw;        // owner rows, first operand  (MODE 0: K_j ; MODE 1: Q_i)
    A *own1 = own0 + TB * ld;       //             second operand (MODE 0: V_j ; MODE 1: dO_i)
    A *swp0 = own1 + TB * ldv;      // swept rows                 (MODE 0: Q_i ; MODE 1: K_j)
    A *swp1 = swp0 + TB * ld;       //                            (MODE 0: dO_i; MODE 1: V_j)
    A *acc0 = swp1 + TB * ldv;      // outputs: MODE 0 dK, MODE 1 dQ
    A *acc1 = acc0 + TB * ld;       //          MODE 0 dV
    A *Ps = acc1 + TB * ldv;        // [query r][key c]
    A *dSs = Ps + TB * TB;
    A *Lq = dSs + TB * TB;          // per query row of the current pairing
    A *Dq = Lq + TB;
    A *Rs = Dq + TB;                // MODE 1: rowsum(P) of the owned query rows (see Lc below)

    const int b = blockIdx.y, h = blockIdx.z, blk = blockIdx.x;
    // NQ queries and NK keys of sequence b; NO = the owned extent, NS = the swept one
    int qst = 0, NQ = a.N, kst = 0, NK = a.N;
    if constexpr (F & kVarlen) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, qst, NQ);
        fa2_varlen_seq(a.cu_k, b, a.total_k, a.max_k, kst, NK);
        if (blk * TB >= (MODE == 0 ? NK : NQ)) return;  // (whole workgroup, before any barrier)
    }
    const int NO = MODE == 0 ? NK : NQ, NS = MODE == 0 ? NQ : NK;
    // kGqa: MODE 0's grid z is the KV head, its query heads are swept below; MODE 1's is the query head
    const int hk = (F & kGqa) && MODE == 1 ? h / a.gqa : h;
    const int64_t kb = F & kVarlen ? (int64_t)kst * a.ks[2] + hk * a.ks[1] : b * a.ks[0] + hk * a.ks[1];
    const int64_t vb = F & kVarlen ? (int64_t)kst * a.vs[2] + hk * a.vs[1] : b * a.vs[0] + hk * a.vs[1];
    const int64_t lb = F & kVarlen ? h * a.ls[1] + qst : b * a.ls[0] + h * a.ls[1];
    // Q, dO, D and the row statistic of one query head: MODE 1 binds its own head, MODE 0 each head it sweeps.
    // Lc, the fp32 / fp64 row statistic: written by the MODE 1 launch (which runs first), read by MODE 0.  The forward stores
    // L in the I/O dtype (kernels.py:108); its rounding scales a whole row of P (bf16: by up to 2^0.125).  The
    // query-owner kernel sees full rows, measures rowsum(P) = 2^(L_true - L_stored) and hands L + log2(rowsum) on.
    int64_t qb, gb;
    long long db;
    A *Lc;
    auto query_head = [&](int hq) {
        if constexpr (F & kVarlen) {
            qb = (int64_t)qst * a.qs[2] + hq * a.qs[1];
            gb = (int64_t)qst * a.dos[2] + hq * a.dos[1];
            db = (long long)hq * a.total_q + qst;
            Lc = (A *)a.D + (long long)a.H * a.total_q + db;
        } else {
            qb = b * a.qs[0] + hq * a.qs[1];
            gb = b * a.dos[0] + hq * a.dos[1];
            db = ((long long)b * a.H + hq) * a.N;
            Lc = (A *)a.D + (long long)gridDim.y * a.H * a.N + db;
        }
    };
    const A c_s = (A)a.c_log2e, scale = (A)a.scale;

    auto load_rows = [&](A *dst, const void *src, int64_t base, const int64_t *st, int row0, int n, int cols, int ldd) {
        for (int e = tid; e < TB * cols; e += 256) {
            const int r = e / cols, x = e % cols, row = row0 + r;
            dst[r * ldd + x] = row < n ? E::load(src, base + (int64_t)row * st[2] + x * st[3]) : (A)0;
        }
    };
    const int own_row0 = blk * TB;
    if (MODE == 0) {
        load_rows(own0, a.K, kb, a.ks, own_row0, NO, d, ld);
        load_rows(own1, a.V, vb, a.vs, own_row0, NO, dv, ldv);
    } else {
        query_head(h);
        load_rows(own0, a.Q, qb, a.qs, own_row0, NO, d, ld);
        load_rows(own1, a.dO, gb, a.dos, own_row0, NO, dv, ldv);
        if (tid < TB) {
            const int row = own_row0 + tid;
            Lq[tid] = row < NO ? E::load(a.L, lb + row) : (A)0;
            Dq[tid] = row < NO ? ((const A *)a.D)[db + row] : (A)0;
            Rs[tid] = (A)0;
        }
    }
    if constexpr (F & kDv) {
        for (int e = tid; e < TB * ld; e += 256) acc0[e] = (A)0;
        for (int e = tid; e < TB * ldv; e += 256) acc1[e] = (A)0;
    } else {
        for (int e = tid; e < TB * ld; e += 256) acc0[e] = acc1[e] = (A)0;
    }
    __syncthreads();

    int wl = a.wl, wr = a.wr, sw_begin, sw_end;
    if constexpr (F & kVarlen) {
        // the sequence's band: a key block meets queries [j0 - wr, j1 + wl], a query block keys [i0 - wl, i1 + wr]
        fa2_varlen_band(NQ, NK, a.causal, a.wl, a.wr, wl, wr);
        const int sw_lo = own_row0 - (MODE == 0 ? wr : wl), sw_hi = own_row0 + TB - 1 + (MODE == 0 ? wl : wr);
        sw_begin = (sw_lo > 0 ? sw_lo : 0) / TB;
        sw_end = (NS == 0 || sw_hi < 0) ? 0 : (sw_hi < NS - 1 ? sw_hi : NS - 1) / TB + 1;  // (no swept row: nothing)
    } else if constexpr (F & kWindow) {
        // window: a key block meets queries [j0 - wr, j1 + wl], a query block keys [i0 - wl, i1 + wr]
        const int sw_lo = own_row0 - (MODE == 0 ? wr : wl), sw_hi = own_row0 + TB - 1 + (MODE == 0 ? wl : wr);
        sw_begin = (sw_lo > 0 ? sw_lo : 0) / TB;
        sw_end = (sw_hi < NS - 1 ? sw_hi : NS - 1) / TB + 1;
    } else {
        const int nsw = (NS + TB - 1) / TB;
        // causal: a key block only meets query rows >= its first key; a query block only keys <= its last row
        sw_begin = (MODE == 0 && a.causal) ? own_row0 / TB : 0;
        sw_end = (MODE == 1 && a.causal) ? ((own_row0 + TB - 1 < NS ? own_row0 + TB - 1 : NS - 1) / TB + 1) : nsw;
    }
    // MODE 0 under kGqa: the g query heads of this KV head, in order, into the same accumulators (otherwise one head, once)
    const int ngq = (F & kGqa) && MODE == 0 ? a.gqa : 1;
    for (int gq = 0; gq < ngq; ++gq) {
        if (MODE == 0) query_head(F & kGqa ? h * a.gqa + gq : h);
        for (int sw = sw_begin; sw < sw_end; ++sw) {
            const int sw_row0 = sw * TB;
            if (MODE == 0) {
                load_rows(swp0, a.Q, qb, a.qs, sw_row0, NS, d, ld);
                load_rows(swp1, a.dO, gb, a.dos, sw_row0, NS, dv, ldv);
                if (tid < TB) {
                    const int row = sw_row0 + tid;
                    Lq[tid] = row < NS ? Lc[row] : (A)0;
                    Dq[tid] = row < NS ? ((const A *)a.D)[db + row] : (A)0;
                }
            } else {
                load_rows(swp0, a.K, kb, a.ks, sw_row0, NS, d, ld);
                load_rows(swp1, a.V, vb, a.vs, sw_row0, NS, dv, ldv);
            }
            __syncthreads();
            if (tid < TB * TB) {  // one (query r, key c) pair per thread
                const int r = tid / TB, c = tid % TB;
                const A *qrow = (MODE == 0 ? swp0 : own0) + r * ld, *krow = (MODE == 0 ? own0 : swp0) + c * ld;
                const A *grow = (MODE == 0 ? swp1 : own1) + r * ldv, *vrow = (MODE == 0 ? own1 : swp1) + c * ldv;
                const int qi = (MODE == 0 ? sw_row0 : own_row0) + r, kj = (MODE == 0 ? own_row0 : sw_row0) + c;
                A s = 0, dp = 0;
                if constexpr (F & kDv) {
                    for (int x = 0; x < d; ++x) s += qrow[x] * krow[x];     // kernels.py:283
                    for (int x = 0; x < dv; ++x) dp += grow[x] * vrow[x];  // :289
                } else {
                    for (int x = 0; x < d; ++x) {
                        s += qrow[x] * krow[x];   // kernels.py:283
                        dp += grow[x] * vrow[x];  // :289
                    }
                }
                A p = exp2_acc<A>(s * c_s - Lq[r]);  // :285
                if constexpr (F & kWindow) {
                    if (qi >= NQ || kj >= NK || kj < qi - wl || kj > qi + wr) p = 0;
                } else {
                    if (qi >= NQ || kj >= NK || (a.causal && kj > qi)) p = 0;
                }
                Ps[r * TB + c] = p;  // unrounded: MODE 1 sums it; the cast of :287 happens where it is consumed
                dSs[r * TB + c] = E::round(p * (dp - Dq[r]) * scale);  // :291
            }
            __syncthreads();
            if (MODE == 1 && tid < TB) {
                A t = 0;
                for (int c = 0; c < TB; ++c) t += Ps[tid * TB + c];
                Rs[tid] += t;
            }
            if constexpr (F & kDv) {
                for (int e = tid; e < TB * d; e += 256) {
                    const int o = e / d, x = e % d;
                    A t = 0;  // MODE 0, o = key c: dK[c] += sum_r dS[r][c] Q[r] (:293); MODE 1, o = query r: dQ[r] += sum_c dS[r][c] K[c] (:317)
                    if (MODE == 0)
                        for (int r = 0; r < TB; ++r) t += dSs[r * TB + o] * swp0[r * ld + x];
                    else
                        for (int c = 0; c < TB; ++c) t += dSs[o * TB + c] * swp0[c * ld + x];
                    acc0[o * ld + x] += t;
                }
                if (MODE == 0)
                    for (int e = tid; e < TB * dv; e += 256) {  // dV[c] += sum_r P[r][c] dO[r]   (:287)
                        const int o = e / dv, x = e % dv;
                        A av = 0;
                        for (int r = 0; r < TB; ++r) av += E::round(Ps[r * TB + o]) * swp1[r * ldv + x];
                        acc1[o * ldv + x] += av;
                    }
            } else {
                for (int e = tid; e < TB * d; e += 256) {
                    const int o = e / d, x = e % d;
                    if (MODE == 0) {  // o = key c:  dV[c] += sum_r P[r][c] dO[r],  dK[c] += sum_r dS[r][c] Q[r]   (:287, :293)
                        A av = 0, ak = 0;
                        for (int r = 0; r < TB; ++r) {
                            av += E::round(Ps[r * TB + o]) * swp1[r * ld + x];
                            ak += dSs[r * TB + o] * swp0[r * ld + x];
                        }
                        acc1[o * ld + x] += av;
                        acc0[o * ld + x] += ak;
                    } else {  // o = query r:  dQ[r] += sum_c dS[r][c] K[c]   (:317)
                        A aq = 0;
                        for (int c = 0; c < TB; ++c) aq += dSs[o * TB + c] * swp0[c * ld + x];
                        acc0[o * ld + x] += aq;
                    }
                }
            }
            __syncthreads();
        }
    }
    if constexpr (F & kVarlen) {
        for (int e = tid; e < TB * d; e += 256) {
            const int o = e / d, x = e % d, row = own_row0 + o;
            if (row >= NO) continue;
            if (MODE == 0) {
                E::store(a.dK, h * a.dks[1] + (int64_t)(kst + row) * a.dks[2] + x * a.dks[3], acc0[o * ld + x]);
                if constexpr (!(F & kDv))
                    E::store(a.dV, h * a.dvs[1] + (int64_t)(kst + row) * a.dvs[2] + x * a.dvs[3], acc1[o * ld + x]);
            } else {  // (a row without a visible key: rowsum 0, dQ 0)
                E::store(a.dQ, h * a.dqs[1] + (int64_t)(qst + row) * a.dqs[2] + x * a.dqs[3],
                         Rs[o] > 0 ? acc0[o * ld + x] / Rs[o] : (A)0);
            }
        }
        if constexpr (F & kDv) {
            if (MODE == 0)
                for (int e = tid; e < TB * dv; e += 256) {
                    const int o = e / dv, x = e % dv, row = own_row0 + o;
                    if (row < NO) E::store(a.dV, h * a.dvs[1] + (int64_t)(kst + row) * a.dvs[2] + x * a.dvs[3], acc1[o * ldv + x]);
                }
        }
        // L = +inf and rowsum 0 would give inf + -inf: such a row keeps +inf, and MODE 0 recomputes P = 0 for it
        if (MODE == 1 && tid < TB && own_row0 + tid < NO) Lc[own_row0 + tid] = Rs[tid] > 0 ? Lq[tid] + log2_acc<A>(Rs[tid]) : (A)INFINITY;
    } else {
        for (int e = tid; e < TB * d; e += 256) {
            const int o = e / d, x = e % d, row = own_row0 + o;
            if (row >= NO) continue;
            if (MODE == 0) {
                E::store(a.dK, b * a.dks[0] + h * a.dks[1] + row * a.dks[2] + x * a.dks[3], acc0[o * ld + x]);
                E::store(a.dV, b * a.dvs[0] + h * a.dvs[1] + row * a.dvs[2] + x * a.dvs[3], acc1[o * ld + x]);
            } else {
                E::store(a.dQ, b * a.dqs[0] + h * a.dqs[1] + row * a.dqs[2] + x * a.dqs[3], acc0[o * ld + x] / Rs[o]);
            }
        }
        if (MODE == 1 && tid < TB && own_row0 + tid < NO) Lc[own_row0 + tid] = Lq[tid] + log2_acc<A>(Rs[tid]);
    }
}

template <typename E, int F> int launch_e(const Fa2BwdProblem &p, GArgs &a) {
    using A = typename E::acc_t;
    const int dv = F & kDv ? p.dv : p.d;
    int TB = 16;
    auto need = [&](int tb) { return (size_t)(3 * tb * (p.d + 1) + 3 * tb * (dv + 1) + 2 * tb * tb + 3 * tb) * sizeof(A); };
    while (TB > 1 && need(TB) > 60 * 1024) TB >>= 1;
    a.TB = TB;
    const size_t smem = need(TB);
    const long long rows = F & kVarlen ? (long long)p.H * p.total_q : (long long)p.B * p.H * p.N;
    if (rows > 0)
        hipLaunchKernelGGL((bwd_D_kernel<E, F>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, p.stream, a, rows);
    // kVarlen: one grid for both modes, blocks past a sequence's owned extent leave at once
    const int gx = ((F & kVarlen ? (p.max_q > p.max_k ? p.max_q : p.max_k) : p.N) + TB - 1) / TB;
    if (gx == 0) return FA2_OK;
    const dim3 grid(gx, p.B, p.H), grid0(gx, p.B, p.H / a.gqa);  // MODE 0: one workgroup per KV head
    hipLaunchKernelGGL((bwd_main_kernel<E, 1, F>), grid, dim3(256), smem, p.stream, a);  // first: leaves Lc for MODE 0
    hipLaunchKernelGGL((bwd_main_kernel<E, 0, F>), grid0, dim3(256), smem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("generic backward launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <int F> int launch_form(const Fa2BwdProblem &p, int gqa) {
    if (p.B > 65535 || p.H > 65535) {
        fa2_set_error("generic backward: B and H must be <= 65535");
        return FA2_ERR_BAD_ARG;
    }
    GArgs a = {};
    a.Q = p.Q; a.K = p.K; a.V = p.V; a.O = p.O; a.dO = p.dO; a.L = p.L;
    a.dQ = p.dQ; a.dK = p.dK; a.dV = p.dV; a.D = p.D;
    for (int k = 0; k < 4; ++k) {
        a.qs[k] = p.qs[k]; a.ks[k] = p.ks[k]; a.vs[k] = p.vs[k]; a.os[k] = p.os[k]; a.dos[k] = p.dos[k];
        a.dqs[k] = p.dqs[k]; a.dks[k] = p.dks[k]; a.dvs[k] = p.dvs[k];
    }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.H = p.H; a.N = p.N; a.d = p.d;
    a.causal = (F & (kWindow | kVarlen)) == kWindow ? 0 : p.causal;  // (a dense window arrives normalised: causal is in its sides)
    if constexpr (F & kWindow) { a.wl = p.wl; a.wr = p.wr; }
    if constexpr (F & kVarlen) {
        a.cu_q = p.cu_q; a.cu_k = p.cu_k; a.max_q = p.max_q; a.max_k = p.max_k; a.total_q = p.total_q; a.total_k = p.total_k;
    }
    a.gqa = gqa;
    if constexpr (F & kDv) a.dv = p.dv;
    a.c_log2e = (double)p.scale * FA2_LOG2E;
    a.scale = (double)p.scale;
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32, F>(p, a);
    case FA2_DTYPE_F16: return launch_e<ElemF16, F>(p, a);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16, F>(p, a);
    case FA2_DTYPE_F64: return launch_e<ElemF64, F>(p, a);
    default: fa2_set_error("backward: dtype enum %d is not supported", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}

}  // namespace

int fa2_bwd_launch_generic(const Fa2BwdProblem &p) { return launch_form<0>(p, 1); }
int fa2_bwd_launch_generic_window(const Fa2BwdProblem &p) { return launch_form<kWindow>(p, 1); }
int fa2_bwd_launch_generic_varlen(const Fa2BwdProblem &p) { return launch_form<kWindow | kVarlen>(p, 1); }
int fa2_bwd_launch_generic_window_gqa(const Fa2BwdProblem &p, int gqa) { return launch_form<kWindow | kGqa>(p, gqa); }
int fa2_bwd_launch_generic_varlen_gqa(const Fa2BwdProblem &p, int gqa) { return launch_form<kWindow | kVarlen | kGqa>(p, gqa); }
int fa2_bwd_launch_generic_varlen_dv(const Fa2BwdProblem &p, int gqa) { return launch_form<kWindow | kVarlen | kGqa | kDv>(p, gqa); }
