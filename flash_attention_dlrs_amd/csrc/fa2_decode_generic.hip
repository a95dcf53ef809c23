// fa2_decode_generic.hip -- the catch-all KV-cache decode kernel (fa2_fwd_kvcache, FA2_KVCACHE_VARIANT_GENERIC): every
// supported dtype (f64, f32, f16, bf16; an fp8 cache under f16 / bf16), any strides, any d in [1, 512], any g * N_q -- and, for
// fa2_fwd_kvcache_mla, d up to 576 with a value head size d_v of its own (V (B, H_kv, S_k, d_v), which may be a view of K: neither
// is written): the score loop runs over d, a lane's output columns come from d_v.  The arithmetic and the work split inside
// a workgroup are fa2_generic.hip's varlen form (16 query rows per workgroup, 4 per wave, lane = key for the scores, lane =
// output column for P.V); on top of it the keys of one sequence are split across workgroups as the MFMA form splits them
// (fa2_decode.h), each (split, row) writing a normalised fp32 partial O_s and its log2-domain L_s to the workspace for the
// combine launch -- or, with one split, O and L directly in the I/O dtype.
//
// Stale cache rows never reach the output: K rows are loaded for keys below the split's end only (<= N_k), masked scores are
// selected to -inf, and the P.V loop stops at the split's end, so no V row past N_k is read at all.
//
// K and V of a KV head are read once per QUERY head here, and a 16-row tile holds N_q useful rows: this is the fallback behind
// fa2_decode_mfma16.hip, correct for any N_q but not a performance path at large N_q.
//
// fp8 cache (fa2_fwd_kvcache_fp8): the element type C of K and V is a template parameter beside E, that of Q, O and L.  An
// e4m3fn / e5m2 element is converted (exactly) as it is loaded; the descales kd, vd at [b, h_kv] are folded: kd into the
// softmax scale, vd into the fp32 normalised output before it is rounded or written as a partial.  C and (d, d_v) are independent:
// fa2_fwd_kvcache_mla_fp8 reaches the fp8 instantiations with d up to 576 and a d_v of its own.
//
// Paged cache (fa2_fwd_kvcache_paged): PAGED is a template parameter as well, K and V a page pool behind a block table, any
// page_size >= 1.  Key j of sequence b is row j % page_size of page table[b][j / page_size], the entry clamped to
// [0, num_blocks - 1] before it becomes an address (a wild entry: a wrong result, never an access outside the pool).  For the
// scores a lane looks up the page of its own key; the P.V loop walks the keys in order and looks the page up once per run of
// keys inside a page.  Only keys below the split's end are looked up, so entries past a sequence's pages are never loaded.
//
// Variable-length queries (fa2_fwd_kvcache_varlen): with cu_q the rows are packed (total_q, H, d), sequence b owns n_q(b) rows
// from its start on (fa2_varlen_seq) and the grid's query tiles cover max_seqlen_q: a tile at or past n_q(b) leaves at once, the
// band is the one of n_q(b) and N_k(b), and rows past n_q(b) -- the next sequence's in the packed layout -- are not stored.
#include <math.h>

#include "fa2_decode.h"
#include "fa2_elem.h"

namespace {

constexpr int kRowsPerWave = 4;
constexpr int kWaves = 4;
constexpr int kBr = kRowsPerWave * kWaves;
constexpr int kBc = 64;  // one key per lane

// fp8 cache elements: one byte, converted to fp32 (exactly) by v_cvt_f32_fp8 / v_cvt_f32_bf8 as it is loaded.
struct CacheF8E4M3 {
    static __device__ __forceinline__ float load(const void *p, int64_t i) {
        return __builtin_amdgcn_cvt_f32_fp8((int)((const uint8_t *)p)[i], 0);
    }
};
struct CacheF8E5M2 {
    static __device__ __forceinline__ float load(const void *p, int64_t i) {
        return __builtin_amdgcn_cvt_f32_bf8((int)((const uint8_t *)p)[i], 0);
    }
};

struct DecodeGenericArgs {
    const void *Q, *K, *V;
    void *O, *L;
    int64_t qs[4], ks[4], vs[4], os[4], ls[2];
    const int32_t *seqlens;
    int H, gqa, N_q, S_k, d, dv, causal, wl, wr, num_splits, nqt;  // dv: columns of V, O and the partials
    float *o_part, *l_part;
    double c_log2e;
    const float *kd, *vd;  // fp8 cache only: descales at [b * kds[0] + h_kv * kds[1]], null = 1
    int64_t kds[2], vds[2];
    const int32_t *table;  // paged cache only: entry [b, i] at b * table_stride + i; ks[0], vs[0] are the block strides
    int64_t table_stride;
    int page_size, num_blocks;
    const int32_t *cu_q;  // packed queries: B + 1 offsets (qs[0] = os[0] = ls[0] = 0), else null
    int total_q, max_q;
};

// grid (num_splits * nqt, B, H); DPL = output columns per lane = ceil(d_v / 64).  E: Q, O, L; C: K, V (E, or an fp8 format).
// PAGED: K and V are a page pool behind a block table.
template <class E, class C, bool PAGED, int DPL>
__global__ __launch_bounds__(kWaves * 64) void fa2_decode_generic_kernel(const DecodeGenericArgs a) {
    using A = typename E::acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    A *q_lds = (A *)smem_raw;              // [kBr][d]
    A *p_lds = q_lds + (size_t)kBr * a.d;  // [kWaves][kRowsPerWave][kBc]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = blockIdx.x / a.nqt, i = blockIdx.x - split * a.nqt;
    const int b = blockIdx.y, h = blockIdx.z;
    const int d = a.d, dv = a.dv;
    int N = a.N_q, start = 0;  // the sequence's query count and its first packed row
    if (a.cu_q) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, start, N);
        if (i * kBr >= N) return;  // no rows: nothing to write, no partials
    }
    int NK, k0, k1;
    fa2_decode_split(a.seqlens, b, a.S_k, a.num_splits, split, NK, k0, k1);
    const int hk = h / a.gqa;
    const int64_t q_off = b * a.qs[0] + h * a.qs[1] + (int64_t)start * a.qs[2];
    const int64_t k_off = (PAGED ? 0 : b * a.ks[0]) + hk * a.ks[1];  // (paged: the page's block term joins per key)
    const int64_t v_off = (PAGED ? 0 : b * a.vs[0]) + hk * a.vs[1];
    const int32_t *tab = PAGED ? a.table + b * a.table_stride : nullptr;  // this sequence's row of the block table

    for (int idx = tid; idx < kBr * d; idx += kWaves * 64) {
        const int r = idx / d, x = idx - r * d;
        int row = i * kBr + r;
        row = row < N ? row : N - 1;
        q_lds[idx] = E::load(a.Q, q_off + (int64_t)row * a.qs[2] + (int64_t)x * a.qs[3]);
    }
    __syncthreads();

    constexpr bool F8 = !__is_same(C, E);
    A c = sizeof(A) == 8 ? (A)a.c_log2e : (A)(float)a.c_log2e;
    A vd = 1;
    if constexpr (F8) {
        c *= fa2_decode_descale(a.kd, a.kds[0], a.kds[1], b, hk);
        vd = fa2_decode_descale(a.vd, a.vds[0], a.vds[1], b, hk);
    }
    const int row0 = i * kBr + wave * kRowsPerWave;
    A m[kRowsPerWave], lsum[kRowsPerWave], o[kRowsPerWave][DPL];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        m[r] = -INFINITY;
        lsum[r] = 0;
#pragma unroll
        for (int cc = 0; cc < DPL; ++cc) o[r][cc] = 0;
    }

    // the keys of this split that the band of the workgroup's 16 rows touches (same trip count for every wave: barriers inside)
    int wl, wr;
    fa2_varlen_band(N, NK, a.causal, a.wl, a.wr, wl, wr);
    const int kbeg = i * kBr - wl > k0 ? i * kBr - wl : k0;
    const int kend = i * kBr + kBr + wr < k1 ? i * kBr + kBr + wr : k1;
    A *p_w = p_lds + (size_t)wave * kRowsPerWave * kBc;

    for (int kt = kbeg; kt < kend; kt += kBc) {
        const int key = kt + lane;
        const bool valid = key < kend;
        A dot[kRowsPerWave];
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) dot[r] = 0;
        if (valid) {
            int64_t kb = k_off + (int64_t)key * a.ks[2];
            if constexpr (PAGED) {  // this lane's key: its page, and its row in the page
                const int pg = key / a.page_size;
                kb = k_off + fa2_decode_page(tab, pg, a.num_blocks) * a.ks[0] + (int64_t)(key - pg * a.page_size) * a.ks[2];
            }
            for (int x = 0; x < d; ++x) {
                const A kx = C::load(a.K, kb + (int64_t)x * a.ks[3]);
#pragma unroll
                for (int r = 0; r < kRowsPerWave; ++r) dot[r] += q_lds[(wave * kRowsPerWave + r) * d + x] * kx;
            }
        }
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            A s = dot[r] * c;
            if (!valid || key < row0 + r - wl || key > row0 + r + wr) s = -INFINITY;  // selected, never multiplied
            const A mx = wave_max(s);
            const A m_new = m[r] > mx ? m[r] : mx;
            // while a row's maximum is -inf, P and the rescale factor are 0 (not exp2(-inf + inf))
            const A m_use = m_new == -INFINITY ? (A)0 : m_new;
            const A p = exp2_acc<A>(s - m_use);
            const A coeff = exp2_acc<A>(m[r] - m_use);
            lsum[r] = coeff * lsum[r] + p;
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) o[r][cc] *= coeff;
            m[r] = m_new;
            p_w[r * kBc + lane] = E::round(p);
        }
        __syncthreads();
        const int kmax = (kend - kt) < kBc ? (kend - kt) : kBc;
        int64_t v_page = 0;  // paged: element offset of row 0 of the current page, looked up once per run of keys inside a page
        int v_row = 0;       //        and the next key's row in it
        for (int kk = 0; kk < kmax; ++kk) {
            int64_t vb = v_off + (int64_t)(kt + kk) * a.vs[2];
            if constexpr (PAGED) {
                if (kk == 0 || v_row == a.page_size) {
                    const int pg = (kt + kk) / a.page_size;
                    v_row = kt + kk - pg * a.page_size;
                    v_page = v_off + fa2_decode_page(tab, pg, a.num_blocks) * a.vs[0];
                }
                vb = v_page + (int64_t)v_row * a.vs[2];
                ++v_row;
            }
            A pr[kRowsPerWave];
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) pr[r] = p_w[r * kBc + kk];
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) {
                    const A v = C::load(a.V, vb + (int64_t)x * a.vs[3]);
#pragma unroll
                    for (int r = 0; r < kRowsPerWave; ++r) o[r][cc] += pr[r] * v;
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int row = row0 + r;
        const A l = wave_sum(lsum[r]);
        if (row >= N) continue;
        if (a.num_splits == 1) {  // a row without a visible key: O = 0, L = +inf
            const int64_t o_off = b * a.os[0] + h * a.os[1] + (int64_t)(start + row) * a.os[2];
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) E::store(a.O, o_off + (int64_t)x * a.os[3], l > 0 ? (F8 ? o[r][cc] / l * vd : o[r][cc] / l) : (A)0);
            }
            if (lane == 0) E::store(a.L, b * a.ls[0] + h * a.ls[1] + start + row, l > 0 ? m[r] + log2_acc<A>(l) : (A)INFINITY);
        } else {  // every (split, row) is written, an empty split as O_s = 0, L_s = -inf: the workspace arrives uninitialised
            const int64_t rows = a.cu_q ? (int64_t)a.total_q * a.H : (int64_t)gridDim.y * a.H * N;
            const int64_t prow = (int64_t)split * rows + (a.cu_q ? (int64_t)(start + row) * a.H + h : ((int64_t)b * a.H + h) * N + row);
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) a.o_part[prow * dv + x] = l > 0 ? (float)(F8 ? o[r][cc] / l * vd : o[r][cc] / l) : 0.0f;
            }
            if (lane == 0) a.l_part[prow] = l > 0 ? (float)(m[r] + log2_acc<A>(l)) : -INFINITY;
        }
    }
}

// More than 64 KiB of dynamic LDS (d > 256 in double) is opted into, once per device and instantiation.
template <class E, class C, bool PAGED, int DPL>
void launch_k(const dim3 &grid, const dim3 &block, size_t smem, hipStream_t stream, const DecodeGenericArgs &a) {
    static Fa2DeviceLatch attr_done;
    if (smem > 64 * 1024 && attr_done.need()) {
        (void)hipFuncSetAttribute((const void *)fa2_decode_generic_kernel<E, C, PAGED, DPL>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(typename E::acc_t) * ((size_t)kBr * 576 + (size_t)kWaves * kRowsPerWave * kBc)));
        attr_done.mark();
    }
    hipLaunchKernelGGL((fa2_decode_generic_kernel<E, C, PAGED, DPL>), grid, block, smem, stream, a);
}

template <class E, class C, bool PAGED> int launch_p(const Fa2DecodeProblem &p, const DecodeGenericArgs &a) {
    const long long gx = (long long)a.num_splits * a.nqt;
    if (gx > 0x7fffffffLL) {
        fa2_set_error("kvcache generic kernel: grid too large (num_splits * ceil(N_q / 16) = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    const dim3 grid((unsigned)gx, p.B, p.H), block(kWaves * 64);
    const size_t smem = sizeof(typename E::acc_t) * ((size_t)kBr * (p.d > p.d_v ? p.d : p.d_v) + (size_t)kWaves * kRowsPerWave * kBc);
    const int dpl = (p.d_v + 63) / 64;
    if (dpl <= 1) launch_k<E, C, PAGED, 1>(grid, block, smem, p.stream, a);
    else if (dpl <= 2) launch_k<E, C, PAGED, 2>(grid, block, smem, p.stream, a);
    else if (dpl <= 4) launch_k<E, C, PAGED, 4>(grid, block, smem, p.stream, a);
    else launch_k<E, C, PAGED, 8>(grid, block, smem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache generic kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <class E, class C = E> int launch_e(const Fa2DecodeProblem &p, const DecodeGenericArgs &a) {
    return p.table ? launch_p<E, C, true>(p, a) : launch_p<E, C, false>(p, a);
}

}  // namespace

int fa2_launch_decode_generic(const Fa2DecodeProblem &p) {
    DecodeGenericArgs a;
    a.Q = p.Q; a.K = p.K; a.V = p.V; a.O = p.O; a.L = p.L;
    for (int k = 0; k < 4; ++k) { a.qs[k] = p.qs[k]; a.ks[k] = p.ks[k]; a.vs[k] = p.vs[k]; a.os[k] = p.os[k]; }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.seqlens = p.seqlens;
    a.H = p.H; a.gqa = p.H / p.H_kv; a.N_q = p.N_q; a.S_k = p.S_k; a.d = p.d; a.dv = p.d_v; a.causal = p.causal; a.wl = p.wl; a.wr = p.wr;
    a.num_splits = p.num_splits;
    a.nqt = (p.N_q + kBr - 1) / kBr;
    a.o_part = p.o_part; a.l_part = p.l_part;
    a.c_log2e = (double)p.scale * FA2_LOG2E;
    a.kd = p.kd; a.vd = p.vd;
    for (int k = 0; k < 2; ++k) { a.kds[k] = p.kds[k]; a.vds[k] = p.vds[k]; }
    a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.cu_q = p.cu_q; a.total_q = p.total_q; a.max_q = p.max_q;  // (N_q = max_q sizes the query tiles)
    if (p.kv_dtype != p.dtype) {  // fp8 cache under 16-bit Q, O, L
        const bool e4 = p.kv_dtype == FA2_DTYPE_F8E4M3;
        if ((e4 || p.kv_dtype == FA2_DTYPE_F8E5M2) && p.dtype == FA2_DTYPE_F16)
            return e4 ? launch_e<ElemF16, CacheF8E4M3>(p, a) : launch_e<ElemF16, CacheF8E5M2>(p, a);
        if ((e4 || p.kv_dtype == FA2_DTYPE_F8E5M2) && p.dtype == FA2_DTYPE_BF16)
            return e4 ? launch_e<ElemBF16, CacheF8E4M3>(p, a) : launch_e<ElemBF16, CacheF8E5M2>(p, a);
        fa2_set_error("kvcache: cache dtype enum %d under dtype enum %d is not supported", p.kv_dtype, p.dtype);
        return FA2_ERR_UNSUPPORTED;
    }
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32>(p, a);
    case FA2_DTYPE_F16: return launch_e<ElemF16>(p, a);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16>(p, a);
    case FA2_DTYPE_F64: return launch_e<ElemF64>(p, a);
    default: fa2_set_error("kvcache: dtype enum %d is not supported", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}
