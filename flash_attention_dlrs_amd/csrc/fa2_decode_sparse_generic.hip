// fa2_decode_sparse_generic.hip -- the catch-all kernel of the sparse latent-cache call (fa2_fwd_kvcache_mla_sparse,
// FA2_KVCACHE_VARIANT_GENERIC): every (sequence, KV head, query position) attends over its own list of key indices.  Every supported
// dtype (f64, f32, f16, bf16; an fp8 cache under f16 / bf16), any strides, d up to 576 with a value head size d_v of its own, a V
// that is a tensor of its own, contiguous or paged with any page size.
//
// fa2_decode_generic.hip gives a workgroup 16 query positions of one head -- 16 different lists.  Here a workgroup owns 16 HEADS of
// one KV group at ONE query position, which share one list: 4 per wave, a last tile with fewer heads computing the group's last head
// again and dropping it.  The grid's x axis is ((b * N_q + position) * num_splits + split) * ceil(g / 16) + head tile, y the KV head.
// Within it the arithmetic is the generic kernel's: lane = slot for the scores, lane = output column for P.V, the online softmax in
// the exp2 domain with masked scores SELECTED to -inf and P rounded to the I/O dtype, fp8 elements converted exactly as they are
// loaded with the descales folded (kd into the softmax scale, vd into the fp32 normalised output), the partial layout and the
// one-split output.
//
// The list.  Split s covers the slots [s c, (s + 1) c) of the list (fa2_decode_split_slots).  For the scores a lane reads the entry
// of its own slot; an entry outside [0, N_k(b)) is no key -- it is never turned into a table index or an address, and its score is
// -inf.  A valid entry's row is position * row stride in the contiguous cache; through a block table row (j % page_size) of page
// table[b][j / page_size], the entry clamped to [0, num_blocks - 1].  The lane leaves the element offset of its V row (or -1) in
// LDS, and the P.V loop walks the 64 slots in order, skipping those that are no key: only listed rows below N_k(b) are ever read,
// and a key listed twice is read and counted twice.
//
// Packed queries (fa2_fwd_kvcache_mla_sparse_varlen).  VQ is a template parameter, instantiated in fa2_decode_sparse_generic_v.hip
// (FA2_DECODE_SPARSE_VARLEN) alone: the x axis runs over total_q packed rows in B * N_q's place, the workgroup finds the sequence
// that owns its row (fa2_varlen_owner: a uniform binary search over cu_q, then fa2_varlen_seq) and takes N_k(b), the table row and the
// descales of that b; a row no sequence owns leaves at once, before any barrier, and writes nothing.  Q, O, L and the lists have no
// batch stride there (the packed row is the position of every address), and the partial row is token * H + head, the combine's for
// cu_q.  Everything else is the fixed form's.
#include <math.h>

#include "fa2_decode.h"
#include "fa2_elem.h"

#ifndef FA2_DECODE_SPARSE_VARLEN
#define FA2_DECODE_SPARSE_VARLEN 0
#endif

namespace {

constexpr bool kVQ = FA2_DECODE_SPARSE_VARLEN != 0;

constexpr int kRowsPerWave = 4;
constexpr int kWaves = 4;
constexpr int kBr = kRowsPerWave * kWaves;  // heads per workgroup
constexpr int kBc = 64;                     // one slot per lane

// fp8 cache elements: one byte, converted to fp32 (exactly) as it is loaded.
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

struct SparseGenericArgs {
    const void *Q, *K, *V;
    void *O, *L;
    int64_t qs[4], ks[4], vs[4], os[4], ls[2], is[4];
    const int32_t *seqlens, *idx;
    int B, H, gqa, N_q, S_k, d, dv, topk, num_splits, nht;  // nht: head tiles of a KV group
    float *o_part, *l_part;
    double c_log2e;
    const float *kd, *vd;  // fp8 cache only: descales at [b * kds[0] + h_kv * kds[1]], null = 1
    int64_t kds[2], vds[2];
    const int32_t *table;  // paged cache: entry [b, i] at b * table_stride + i; ks[0], vs[0] are the block strides.  Null: contiguous
    int64_t table_stride;
    int page_size, num_blocks;
    const int32_t *cu_q;  // VQ only: B + 1 offsets into the packed rows; qs[0] = os[0] = ls[0] = is[0] = 0, N_q holds max_seqlen_q
    int total_q;
};

// grid (B * N_q * num_splits * nht, H_kv), VQ: total_q in B * N_q's place; DPL = output columns per lane = ceil(d_v / 64).  E: Q, O, L; C: K, V (E, or an fp8 format).
template <class E, class C, int DPL, bool VQ>
__global__ __launch_bounds__(kWaves * 64) void fa2_decode_sparse_generic_kernel(const SparseGenericArgs a) {
    using A = typename E::acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int64_t *v_lds = (int64_t *)smem_raw;               // [kWaves][kBc]: a slot's V row (element offset), -1 = no key
    A *q_lds = (A *)(v_lds + kWaves * kBc);             // [kBr][d]
    A *p_lds = q_lds + (size_t)kBr * a.d;               // [kWaves][kRowsPerWave][kBc]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bx = blockIdx.x;
    const int per = a.num_splits * a.nht, tok = bx / per;
    bx -= tok * per;
    const int split = bx / a.nht, ht = bx - split * a.nht;
    int b = tok / a.N_q, qi = tok - b * a.N_q;
    if constexpr (VQ) {  // tok < total_q is a packed row: its owner, or nothing to do (uniform: before any barrier)
        int st, n;
        if (!fa2_varlen_owner(a.cu_q, a.B, a.total_q, a.N_q, tok, b, st, n)) return;
        qi = tok;
    }
    const int hk = blockIdx.y;
    const int d = a.d, dv = a.dv, g = a.gqa;
    int NK, s0, s1;
    fa2_decode_split_slots(a.seqlens, b, a.S_k, a.topk, a.num_splits, split, NK, s0, s1);
    const bool paged = a.table != nullptr;
    const int64_t k_off = (paged ? 0 : b * a.ks[0]) + hk * a.ks[1];  // (paged: the page's block term joins per key)
    const int64_t v_off = (paged ? 0 : b * a.vs[0]) + hk * a.vs[1];
    const int32_t *tab = paged ? a.table + b * a.table_stride : nullptr;  // this sequence's row of the block table
    const int32_t *ip = a.idx + b * a.is[0] + hk * a.is[1] + qi * a.is[2];

    for (int idx = tid; idx < kBr * d; idx += kWaves * 64) {
        const int r = idx / d, x = idx - r * d;
        int hg = ht * kBr + r;
        hg = hg < g ? hg : g - 1;
        q_lds[idx] = E::load(a.Q, b * a.qs[0] + (int64_t)(hk * g + hg) * a.qs[1] + (int64_t)qi * a.qs[2] + (int64_t)x * a.qs[3]);
    }
    __syncthreads();

    constexpr bool F8 = !__is_same(C, E);
    A c = sizeof(A) == 8 ? (A)a.c_log2e : (A)(float)a.c_log2e;
    A vd = 1;
    if constexpr (F8) {
        c *= fa2_decode_descale(a.kd, a.kds[0], a.kds[1], b, hk);
        vd = fa2_decode_descale(a.vd, a.vds[0], a.vds[1], b, hk);
    }
    const int row0 = ht * kBr + wave * kRowsPerWave;  // this wave's first head of the group
    A m[kRowsPerWave], lsum[kRowsPerWave], o[kRowsPerWave][DPL];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        m[r] = -INFINITY;
        lsum[r] = 0;
#pragma unroll
        for (int cc = 0; cc < DPL; ++cc) o[r][cc] = 0;
    }
    A *p_w = p_lds + (size_t)wave * kRowsPerWave * kBc;
    int64_t *v_w = v_lds + wave * kBc;

    for (int st = s0; st < s1; st += kBc) {  // (the same trip count for every wave: barriers inside)
        const int slot = st + lane;
        int j = -1;
        if (slot < s1) j = ip[slot * a.is[3]];
        const bool valid = j >= 0 && j < NK;  // an entry that is no key: never an address
        A dot[kRowsPerWave];
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) dot[r] = 0;
        int64_t vb = -1;
        if (valid) {
            int64_t kb = k_off + (int64_t)j * a.ks[2];
            vb = v_off + (int64_t)j * a.vs[2];
            if (paged) {  // this lane's key: its page, and its row in the page
                const int pg = j / a.page_size;
                const int64_t e = fa2_decode_page(tab, pg, a.num_blocks), row = j - pg * a.page_size;
                kb = k_off + e * a.ks[0] + row * a.ks[2];
                vb = v_off + e * a.vs[0] + row * a.vs[2];
            }
            for (int x = 0; x < d; ++x) {
                const A kx = C::load(a.K, kb + (int64_t)x * a.ks[3]);
#pragma unroll
                for (int r = 0; r < kRowsPerWave; ++r) dot[r] += q_lds[(wave * kRowsPerWave + r) * d + x] * kx;
            }
        }
        v_w[lane] = vb;
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            A s = dot[r] * c;
            if (!valid) s = -INFINITY;  // selected, never multiplied
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
        const int smax = (s1 - st) < kBc ? (s1 - st) : kBc;
        for (int kk = 0; kk < smax; ++kk) {
            const int64_t vr = v_w[kk];
            if (vr < 0) continue;  // no key: its P is 0 and its row is not read (uniform)
            A pr[kRowsPerWave];
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) pr[r] = p_w[r * kBc + kk];
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) {
                    const A v = C::load(a.V, vr + (int64_t)x * a.vs[3]);
#pragma unroll
                    for (int r = 0; r < kRowsPerWave; ++r) o[r][cc] += pr[r] * v;
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int hg = row0 + r;
        const A l = wave_sum(lsum[r]);
        if (hg >= g) continue;
        const int h = hk * g + hg;
        if (a.num_splits == 1) {  // a row without a valid entry: O = 0, L = +inf
            const int64_t o_off = b * a.os[0] + h * a.os[1] + (int64_t)qi * a.os[2];
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) E::store(a.O, o_off + (int64_t)x * a.os[3], l > 0 ? (F8 ? o[r][cc] / l * vd : o[r][cc] / l) : (A)0);
            }
            if (lane == 0) E::store(a.L, b * a.ls[0] + h * a.ls[1] + qi, l > 0 ? m[r] + log2_acc<A>(l) : (A)INFINITY);
        } else {  // every (split, row) is written, an empty split as O_s = 0, L_s = -inf: the workspace arrives uninitialised
            const int64_t rows = VQ ? (int64_t)a.total_q * a.H : (int64_t)a.B * a.H * a.N_q;
            const int64_t prow = (int64_t)split * rows + (VQ ? (int64_t)qi * a.H + h : ((int64_t)b * a.H + h) * a.N_q + qi);
#pragma unroll
            for (int cc = 0; cc < DPL; ++cc) {
                const int x = lane + 64 * cc;
                if (x < dv) a.o_part[prow * dv + x] = l > 0 ? (float)(F8 ? o[r][cc] / l * vd : o[r][cc] / l) : 0.0f;
            }
            if (lane == 0) a.l_part[prow] = l > 0 ? (float)(m[r] + log2_acc<A>(l)) : -INFINITY;
        }
    }
}

size_t smem_bytes(size_t acc, int d) { return sizeof(int64_t) * kWaves * kBc + acc * ((size_t)kBr * d + (size_t)kWaves * kRowsPerWave * kBc); }

// More than 64 KiB of dynamic LDS (d > 256 in double) is opted into, once per device and instantiation.
template <class E, class C, int DPL>
void launch_k(const dim3 &grid, const dim3 &block, size_t smem, hipStream_t stream, const SparseGenericArgs &a) {
    static Fa2DeviceLatch attr_done;
    if (smem > 64 * 1024 && attr_done.need()) {
        (void)hipFuncSetAttribute((const void *)fa2_decode_sparse_generic_kernel<E, C, DPL, kVQ>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)smem_bytes(sizeof(typename E::acc_t), 576));
        attr_done.mark();
    }
    hipLaunchKernelGGL((fa2_decode_sparse_generic_kernel<E, C, DPL, kVQ>), grid, block, smem, stream, a);
}

template <class E, class C = E> int launch_e(const Fa2DecodeProblem &p, const SparseGenericArgs &a) {
    const long long gx = (kVQ ? (long long)p.total_q : (long long)p.B * p.N_q) * a.num_splits * a.nht;
    if (gx > 0x7fffffffLL) {
        fa2_set_error(kVQ ? "kvcache mla sparse varlen: grid too large (total_q * num_splits * ceil(g / 16) = %lld)"
                          : "kvcache mla sparse: grid too large (B * N_q * num_splits * ceil(g / 16) = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    const dim3 grid((unsigned)gx, p.H_kv), block(kWaves * 64);
    const size_t smem = smem_bytes(sizeof(typename E::acc_t), p.d);
    const int dpl = (p.d_v + 63) / 64;
    if (dpl <= 1) launch_k<E, C, 1>(grid, block, smem, p.stream, a);
    else if (dpl <= 2) launch_k<E, C, 2>(grid, block, smem, p.stream, a);
    else if (dpl <= 4) launch_k<E, C, 4>(grid, block, smem, p.stream, a);
    else launch_k<E, C, 8>(grid, block, smem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache mla sparse generic kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

}  // namespace

#if FA2_DECODE_SPARSE_VARLEN
int fa2_launch_decode_sparse_generic_v(const Fa2DecodeProblem &p) {
#else
int fa2_launch_decode_sparse_generic(const Fa2DecodeProblem &p) {
#endif
    SparseGenericArgs a;
    a.Q = p.Q; a.K = p.K; a.V = p.V; a.O = p.O; a.L = p.L;
    for (int k = 0; k < 4; ++k) { a.qs[k] = p.qs[k]; a.ks[k] = p.ks[k]; a.vs[k] = p.vs[k]; a.os[k] = p.os[k]; a.is[k] = p.is[k]; }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.seqlens = p.seqlens; a.idx = p.indices;
    a.B = p.B; a.H = p.H; a.gqa = p.H / p.H_kv; a.N_q = p.N_q; a.S_k = p.S_k; a.d = p.d; a.dv = p.d_v; a.topk = p.topk;
    a.num_splits = p.num_splits;
    a.nht = (a.gqa + kBr - 1) / kBr;
    a.o_part = p.o_part; a.l_part = p.l_part;
    a.c_log2e = (double)p.scale * FA2_LOG2E;
    a.kd = p.kd; a.vd = p.vd;
    for (int k = 0; k < 2; ++k) { a.kds[k] = p.kds[k]; a.vds[k] = p.vds[k]; }
    a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.cu_q = p.cu_q; a.total_q = p.total_q;
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
