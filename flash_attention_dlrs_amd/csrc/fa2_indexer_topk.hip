// fa2_indexer_topk.hip -- the selection of the MLA indexer (fa2_topk_indices): per (sequence, query position) the min(topk, n) of its
// n candidate logits that come first under (value descending, position ascending), emitted in ascending position, the rest of the
// row -1.
//
// One workgroup of 1,024 threads per row.  A row with n <= topk writes the identity prefix without reading a logit.  Otherwise:
//
//   1. Radix select over an order-preserving 32-bit image of the values (-0.0 canonicalised to +0.0, a NaN to -inf's image; then
//      the usual flip: negative values inverted, the others with the sign bit set, so unsigned order = numeric order).  Four passes
//      of eight bits from the top: an LDS histogram of the digit over the candidates that match the prefix found so far, then one
//      thread walks the 256 bins from the highest down to the bin that holds the topk-th largest.  The bins are integer counts:
//      the order in which the LDS adds arrive cannot change them.  After four passes the prefix is the threshold image T, and
//      `take` of the candidates equal to T belong to the list.
//   2. One ordered compaction pass.  The row is walked in position order, 1,024 candidates a step; a wave's ballots give each lane
//      the count of candidates above T and equal to T before it in the wave, the 16 waves' totals go through LDS and are added in
//      wave order, and the running totals carry over the steps.  A candidate above T lands at slot (above before it) + min(equal
//      before it, take); one equal to T with fewer than `take` equals before it at (above before it) + (equal before it).  The slot
//      is a function of the logits alone, and slots ascend with the position.
//
// Only entries j < n(b, qi) of a row are read.  Stores are plain vector stores.
//
// Packed queries (fa2_topk_indices_varlen).  VQ is a template parameter, instantiated in fa2_indexer_topk_v.hip (FA2_INDEXER_VARLEN)
// alone: one workgroup per packed row, which finds the sequence that owns it (fa2_varlen_owner: a uniform binary search over cu_q,
// then fa2_varlen_seq) and counts its candidates with n_q(b) in N_q's place; a row no sequence owns leaves at once and writes
// nothing.  The logits row and the list are the packed row's (no batch stride).  The rest is the fixed form's.
#include "fa2_indexer.h"

#ifndef FA2_INDEXER_VARLEN
#define FA2_INDEXER_VARLEN 0
#endif

namespace {

constexpr bool kVQ = FA2_INDEXER_VARLEN != 0;

constexpr int kThreads = 1024, kWaves = kThreads / 64;

__device__ __forceinline__ uint32_t image(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;  // NaN ranks as -inf
    if (u == 0x80000000u) u = 0;                           // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool VQ> __global__ __launch_bounds__(kThreads) void fa2_topk_indices_kernel(const Fa2IndexerProblem a) {
    __shared__ int hist[256];
    __shared__ int wsum[kWaves];
    __shared__ uint32_t s_prefix;
    __shared__ int s_rem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x / a.N_q, qi = blockIdx.x - b * a.N_q, N_q = a.N_q, row = qi;  // row: of the logits and the lists within b's
    if constexpr (VQ) {  // blockIdx.x < total_q is a packed row: its owner, or nothing to do (uniform: before any barrier)
        int start;
        row = blockIdx.x;
        if (!fa2_varlen_owner(a.cu_q, a.B, a.total_q, a.max_q, row, b, start, N_q)) return;
        qi = row - start;
    }
    const int n = fa2_indexer_count(a.seqlens, b, a.S_k, N_q, qi, a.causal);
    int32_t *out = a.idx + b * a.is[0] + (int64_t)row * a.is[1];
    if (n <= a.topk) {  // the identity prefix, no logit read
        for (int s = tid; s < a.topk; s += kThreads) out[(int64_t)s * a.is[2]] = s < n ? s : -1;
        return;
    }
    const float *lg = a.LG + b * a.lgs[0] + (int64_t)row * a.lgs[1];

    // ---- 1. the threshold image: the topk-th largest
    uint32_t prefix = 0, mask = 0;
    int rem = a.topk;  // how many of the candidates matching the prefix belong to the list
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += kThreads) {
            const uint32_t im = image(lg[(int64_t)j * a.lgs[2]]);
            if ((im & mask) == prefix) atomicAdd(&hist[(im >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int above = 0, dgt = 255;
            for (; dgt > 0; --dgt) {
                if (above + hist[dgt] >= rem) break;
                above += hist[dgt];
            }
            s_prefix = prefix | ((uint32_t)dgt << shift);
            s_rem = rem - above;
        }
        __syncthreads();
        prefix = s_prefix;
        rem = s_rem;
        mask |= 255u << shift;
    }
    const uint32_t T = prefix;
    const int take = rem;  // >= 1

    // ---- 2. ordered compaction
    int base_gt = 0, base_eq = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j0 = 0; j0 < n; j0 += kThreads) {  // (the same trip count for every thread: barriers inside)
        const int j = j0 + tid;
        const uint32_t im = j < n ? image(lg[(int64_t)j * a.lgs[2]]) : 0u;
        const bool gt = j < n && im > T, eq = j < n && im == T;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        if (lane == 0) wsum[wave] = __popcll(bg) | (__popcll(be) << 16);  // (each <= 64)
        __syncthreads();
        int og = 0, oe = 0, tg = 0, te = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int v = wsum[w], vg = v & 0xffff, ve = v >> 16;
            if (w < wave) {
                og += vg;
                oe += ve;
            }
            tg += vg;
            te += ve;
        }
        const int gt_before = base_gt + og + __popcll(bg & below), eq_before = base_eq + oe + __popcll(be & below);
        // (above in all + take = topk, so a slot is < topk; the test keeps a row that changed between the passes inside its list)
        const int slot = gt_before + (eq_before < take ? eq_before : take);
        if ((gt || (eq && eq_before < take)) && slot < a.topk) out[(int64_t)slot * a.is[2]] = j;
        base_gt += tg;
        base_eq += te;
        __syncthreads();
    }
}

}  // namespace

#if FA2_INDEXER_VARLEN
int fa2_launch_topk_indices_v(const Fa2IndexerProblem &p) {
#else
int fa2_launch_topk_indices(const Fa2IndexerProblem &p) {
#endif
    const long long gx = kVQ ? (long long)p.total_q : (long long)p.B * p.N_q;
    if (gx > 0x7fffffffLL) {
        fa2_set_error("topk indices: grid too large (B * N_q = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(fa2_topk_indices_kernel<kVQ>, dim3((unsigned)gx), dim3(kThreads), 0, p.stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("topk indices kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}
