// fa2_indexer_generic.hip -- the catch-all score kernel of the MLA indexer (fa2_mla_indexer_logits, FA2_INDEXER_VARIANT_GENERIC):
// f32, f16, bf16 (an fp8 cache under f16 / bf16), any strides, any d_I up to 576, any H_I, contiguous or paged with any page size.
//
// Lane = key.  A workgroup of 256 threads owns 256 consecutive keys of one (sequence, query position); the grid is
// (key tiles * N_q, B), the position running fastest.  A thread walks the heads four at a time: one pass over its key row (fp8
// elements converted exactly as they are loaded) feeds four dot products in fp32, whose Q elements are uniform over the workgroup;
// then ReLU, the weights and the running head sum.  k_scale[j] multiplies the sum once.  Keys at and past the position's candidate
// count are neither read nor written, and a tile wholly past it leaves at once.
//
// Packed queries (fa2_mla_indexer_logits_varlen).  VQ is a template parameter, instantiated in fa2_indexer_generic_v.hip
// (FA2_INDEXER_VARLEN) alone: the grid is (key tiles * max_seqlen_q, B), the block takes its sequence's start and n_q(b) from cu_q
// (fa2_varlen_seq), leaves at once when its position is at or past n_q(b), counts the candidates with n_q(b) in N_q's place and
// addresses Q, W and the logits at packed row start + position (no batch stride).
#include "fa2_decode.h"
#include "fa2_elem.h"
#include "fa2_indexer.h"

#ifndef FA2_INDEXER_VARLEN
#define FA2_INDEXER_VARLEN 0
#endif

namespace {

constexpr bool kVQ = FA2_INDEXER_VARLEN != 0;

constexpr int kThreads = 256;
constexpr int kHeads = 4;  // heads per pass over the key row

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

// E: q_idx; C: k_idx (E, or an fp8 format)
template <class E, class C, bool VQ> __global__ __launch_bounds__(kThreads) void fa2_indexer_generic_kernel(const Fa2IndexerProblem a) {
    unsigned bx = blockIdx.x;
    if constexpr (VQ) {  // sequence b takes its blocks rotated by b: the live blocks of short sequences do not sit max_seqlen_q ids
        bx += blockIdx.y % gridDim.x;  // apart on one XCD (fa2_indexer_mfma16.hip has the measurement); a bijection of the same grid
        bx -= bx >= gridDim.x ? gridDim.x : 0;
    }
    const int kt = (int)bx / a.N_q, b = blockIdx.y;
    const int qi = (int)bx - kt * a.N_q;
    int N_q = a.N_q, row = qi;  // row: of Q, W and the logits within b's (VQ: the packed row, no batch stride)
    if constexpr (VQ) {
        int start;
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, start, N_q);
        if (qi >= N_q) return;  // (uniform)
        row = start + qi;       // < total_q
    }
    const int cnt = fa2_indexer_count(a.seqlens, b, a.S_k, N_q, qi, a.causal);
    const int j = kt * kThreads + threadIdx.x;
    if (j >= cnt) return;  // key j < cnt <= N_k(b) <= capacity: its page index is below max_blocks
    int64_t kb, sb;
    if (a.table) {
        const int pg = j / a.page_size;
        const int64_t e = fa2_decode_page(a.table + b * a.table_stride, pg, a.num_blocks), row = j - pg * a.page_size;
        kb = e * a.ks[0] + row * a.ks[1];
        sb = e * a.kss[0] + row * a.kss[1];
    } else {
        kb = b * a.ks[0] + (int64_t)j * a.ks[1];
        sb = b * a.kss[0] + (int64_t)j * a.kss[1];
    }
    const int64_t qb = b * a.qs[0] + (int64_t)row * a.qs[2];
    float sum = 0.0f;
    for (int h0 = 0; h0 < a.H; h0 += kHeads) {
        int64_t qh[kHeads];
#pragma unroll
        for (int r = 0; r < kHeads; ++r) qh[r] = qb + (int64_t)(h0 + r < a.H ? h0 + r : a.H - 1) * a.qs[1];  // (past H_I: the last head, dropped)
        float dot[kHeads] = {};
        for (int x = 0; x < a.d; ++x) {
            const float kx = C::load(a.K, kb + (int64_t)x * a.ks[2]);
#pragma unroll
            for (int r = 0; r < kHeads; ++r) dot[r] += E::load(a.Q, qh[r] + (int64_t)x * a.qs[3]) * kx;
        }
#pragma unroll
        for (int r = 0; r < kHeads; ++r)
            if (h0 + r < a.H) sum += a.W[b * a.ws[0] + (int64_t)(h0 + r) * a.ws[1] + (int64_t)row * a.ws[2]] * fmaxf(dot[r], 0.0f);
    }
    a.LG[b * a.lgs[0] + (int64_t)row * a.lgs[1] + (int64_t)j * a.lgs[2]] = a.KS ? sum * a.KS[sb] : sum;
}

template <class E, class C = E> int launch_e(const Fa2IndexerProblem &p) {
    const long long gx = (long long)((p.S_k + kThreads - 1) / kThreads) * p.N_q;
    if (gx > 0x7fffffffLL) {
        fa2_set_error("mla indexer: grid too large (key tiles * N_q = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL((fa2_indexer_generic_kernel<E, C, kVQ>), dim3((unsigned)gx, p.B), dim3(kThreads), 0, p.stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("mla indexer generic kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

}  // namespace

#if FA2_INDEXER_VARLEN
int fa2_launch_indexer_generic_v(const Fa2IndexerProblem &p) {
#else
int fa2_launch_indexer_generic(const Fa2IndexerProblem &p) {
#endif
    if (p.k_dtype != p.dtype) {  // fp8 cache under 16-bit q_idx (the entry point has checked the pair)
        const bool e4 = p.k_dtype == FA2_DTYPE_F8E4M3;
        if (p.dtype == FA2_DTYPE_F16) return e4 ? launch_e<ElemF16, CacheF8E4M3>(p) : launch_e<ElemF16, CacheF8E5M2>(p);
        return e4 ? launch_e<ElemBF16, CacheF8E4M3>(p) : launch_e<ElemBF16, CacheF8E5M2>(p);
    }
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32>(p);
    case FA2_DTYPE_F16: return launch_e<ElemF16>(p);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16>(p);
    default: fa2_set_error("mla indexer: dtype enum %d is not supported", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}
