// fa2_indexer_topk_split.hip -- the selection of the MLA indexer with a row split over several workgroups (fa2_topk_indices_split):
// the lists of fa2_indexer_topk.hip, byte for byte, for long rows at few rows, where one workgroup per row leaves the chip idle.
//
// Split s of a row covers the positions [s * chunk, (s + 1) * chunk) below the row's candidate count n; a workgroup whose range
// starts at or past n leaves at once (uniform, before any barrier), and so does every workgroup of a row with n <= topk but split 0
// of the last launch, which writes the identity prefix without reading a logit.  Six launches on the call's stream, the grid of all
// but the first (splits, rows), 1,024 threads a workgroup; no workgroup waits for another inside a launch:
//
//   0. Clear the row's three histograms (a kernel, not a memset node: the call can be captured in a graph).
//   1. Three digit passes over the order-preserving 32-bit image of the values (fa2_indexer_topk.hip's: -0.0 = +0.0, a NaN ranks as
//      -inf), 11, 11 and 10 bits from the top.  A pass after the first DERIVES the prefix found so far and the count still to take
//      from the histograms of the passes before it: every thread holds two bins, a suffix sum by shuffles inside the waves and one
//      exchange of the 16 wave totals through LDS gives each bin the count above it, and the one thread whose bin holds the rem-th
//      largest announces it.  All histograms are loaded before the first scan, so the scans wait for memory once.  Every workgroup
//      of a row computes the same integers.  Then the workgroup streams its chunk -- 16-byte loads, four in flight a thread, where
//      the column stride is 1, from the first 16-byte boundary of the chunk on, scalar loads for the head, the tail and strided rows
//      -- counts the digit of every candidate that matches the prefix in an LDS histogram and adds its non-zero bins to the row's
//      histogram in the workspace with integer atomics whose results are unused.
//   2. The count pass: the same streaming body with the full threshold image T; the chunk's counts of candidates above T and equal
//      to T go to cnt[row][split], one plain 8-byte store.
//   3. Emit: a workgroup re-derives T and take, one wave adds the counts of the splits before it, and the ordered compaction of
//      fa2_indexer_topk.hip (ballots, wave totals through LDS in wave order) runs over its chunk from those bases.
//
// Only integer counts are accumulated: the order in which the atomics arrive cannot change a bin.  No floating-point reduction.
// The workspace may hold anything: the histograms are cleared by launch 0, and a count pair is read only from a split that wrote it
// (a split before one that holds candidates holds candidates).
//
// Packed queries: VQ is a template parameter, instantiated in fa2_indexer_topk_split_v.hip (FA2_INDEXER_VARLEN) alone, as
// fa2_indexer_topk.hip's: blockIdx.y is the packed row, a row no sequence owns leaves at once and writes nothing.
#include "fa2_indexer.h"

#ifndef FA2_INDEXER_VARLEN
#define FA2_INDEXER_VARLEN 0
#endif

namespace {

constexpr bool kVQ = FA2_INDEXER_VARLEN != 0;

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kInFlight = 4;  // 16-byte loads a thread issues before it looks at the first

// digit pass p: its shift, its bins, where its histogram starts in the row's kTopkBins
constexpr int dshift(int p) { return p == 0 ? 21 : (p == 1 ? 10 : 0); }
constexpr int dbins(int p) { return p == 2 ? kTopkBins2 : kTopkBins0; }
constexpr int doff(int p) { return p * kTopkBins0; }
static_assert(kTopkBins0 == kTopkBins1 && dbins(0) == 1 << (32 - dshift(0)) && dbins(1) == 1 << (dshift(0) - dshift(1)) &&
              dbins(2) == 1 << dshift(1) && 2 * kThreads >= kTopkBins0, "11 + 11 + 10 bits, two bins a thread");

struct SplitArgs {
    int32_t *hist;  // (rows, kTopkBins)
    int32_t *cnt;   // (rows, splits, 2): above T, equal to T
    int32_t splits, chunk;
};

__device__ __forceinline__ uint32_t image(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;  // NaN ranks as -inf
    if (u == 0x80000000u) u = 0;                           // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Row {
    int r, n, lo, hi;  // the row of the grid, its candidates, this split's positions [lo, hi) (hi <= n)
    const float *lg;
    int32_t *out;
};

// This workgroup's row and range; false for a packed row no sequence owns (uniform).
template <bool VQ> __device__ __forceinline__ bool split_row(const Fa2IndexerProblem &a, const SplitArgs &w, Row &R) {
    R.r = blockIdx.y;
    int b = R.r / a.N_q, qi = R.r - b * a.N_q, N_q = a.N_q, row = qi;
    if constexpr (VQ) {
        int start;
        row = R.r;
        if (!fa2_varlen_owner(a.cu_q, a.B, a.total_q, a.max_q, row, b, start, N_q)) return false;
        qi = row - start;
    }
    R.n = fa2_indexer_count(a.seqlens, b, a.S_k, N_q, qi, a.causal);
    R.lo = (int)blockIdx.x * w.chunk;  // (< S_k: the host's clamp)
    R.hi = R.lo + w.chunk < R.n ? R.lo + w.chunk : R.n;
    R.lg = a.LG + b * a.lgs[0] + (int64_t)row * a.lgs[1];
    R.out = a.idx + b * a.is[0] + (int64_t)row * a.is[1];
    return true;
}

template <class T> __device__ __forceinline__ T wave_sum_to_lane0(T x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
    return x;
}

// The scans' LDS: a slot per stage, so no stage waits for the readers of the one before it.
struct Scan {
    int wtot[3][kWaves];
    int dig[3], rem[3];
};

// The bin that holds the rem-th largest of a histogram, counted from the top bin down, and how many of that bin's candidates still
// belong: thread t holds bins 2 t (v0) and 2 t + 1 (v1), zeros past the histogram's end.  The counts above a bin: the threads after
// t in its wave by a suffix sum of shuffles, the waves after it from LDS.  Exactly one bin has above < rem <= above + count when the
// histogram counts rem candidates at least; otherwise (a row rewritten between the launches) bin 0 and rem as it came.
__device__ __forceinline__ void find_bin(int v0, int v1, int stage, Scan &S, int &dig, int &rem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int x = v0 + v1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_down(x, off);
        if (lane + off < 64) x += y;
    }
    if (lane == 0) S.wtot[stage][wave] = x;
    if (tid == 0) {
        S.dig[stage] = 0;
        S.rem[stage] = rem;
    }
    __syncthreads();
    int above = x - (v0 + v1);
#pragma unroll
    for (int k = 1; k < kWaves; ++k)
        if (k > wave) above += S.wtot[stage][k];
    if (above < rem && rem <= above + v1) {
        S.dig[stage] = 2 * tid + 1;
        S.rem[stage] = rem - above;
    } else if (above + v1 < rem && rem <= above + v1 + v0) {
        S.dig[stage] = 2 * tid;
        S.rem[stage] = rem - above - v1;
    }
    __syncthreads();
    dig = S.dig[stage];
    rem = S.rem[stage];
}

// The prefix of the image after P digit passes and the count still to take, from the row's histograms `h`: after three, the
// threshold image T and `take`.
template <int P> __device__ __forceinline__ void derive(const int32_t *h, int topk, Scan &S, uint32_t &prefix, int &rem) {
    const int tid = threadIdx.x;
    int2 v[P > 0 ? P : 1];
#pragma unroll
    for (int p = 0; p < P; ++p)
        v[p] = 2 * tid < dbins(p) ? reinterpret_cast<const int2 *>(h + doff(p))[tid] : int2{0, 0};
    prefix = 0;
    rem = topk;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        int dig;
        find_bin(v[p].x, v[p].y, p, S, dig, rem);
        prefix |= (uint32_t)dig << dshift(p);
    }
}

// f(image) for every candidate of [lo, hi), in no order.  No barrier inside; the branches are uniform.
template <class F> __device__ __forceinline__ void stream(const float *lg, int64_t cs, int lo, int hi, F &&f) {
    const int tid = threadIdx.x;
    if (cs != 1) {
        for (int j = lo + tid; j < hi; j += kThreads) f(image(lg[(int64_t)j * cs]));
        return;
    }
    const float *p = lg + lo;
    const int len = hi - lo;
    int head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;  // elements before the first 16-byte boundary
    head = head < len ? head : len;
    const int nq = (len - head) >> 2, tail = head + 4 * nq;  // whole quads below hi <= n, then at most three elements
    if (tid < head) f(image(p[tid]));
    if (tail + tid < len) f(image(p[tail + tid]));
    const float4 *q4 = reinterpret_cast<const float4 *>(p + head);
    for (int q = tid; q < nq; q += kInFlight * kThreads) {
        float4 v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) v[u] = q + u * kThreads < nq ? q4[q + u * kThreads] : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
            if (q + u * kThreads < nq) {
                f(image(v[u].x));
                f(image(v[u].y));
                f(image(v[u].z));
                f(image(v[u].w));
            }
    }
}

__global__ __launch_bounds__(256) void fa2_topk_split_zero_kernel(int4 *hist) {
    hist[(int64_t)blockIdx.y * (kTopkBins / 4) + blockIdx.x * 256 + threadIdx.x] = int4{0, 0, 0, 0};
}
static_assert(kTopkBins % (4 * 256) == 0, "whole workgroups of 16-byte stores");

// P = 0, 1, 2: digit pass P.  P = 3: the count pass.
template <bool VQ, int P> __global__ __launch_bounds__(kThreads) void fa2_topk_split_pass_kernel(const Fa2IndexerProblem a, const SplitArgs w) {
    __shared__ int lh[P < 3 ? dbins(P) : 2 * kWaves];
    __shared__ Scan S;
    const int tid = threadIdx.x;
    Row R;
    if (!split_row<VQ>(a, w, R)) return;
    if (R.n <= a.topk || R.lo >= R.n) return;
    int32_t *h = w.hist + (int64_t)R.r * kTopkBins;
    uint32_t prefix;
    int rem;
    derive<P>(h, a.topk, S, prefix, rem);
    if constexpr (P < 3) {
        constexpr int NB = dbins(P), SH = dshift(P);
        constexpr uint32_t mask = P == 0 ? 0u : ~0u << dshift(P > 0 ? P - 1 : 0);
        for (int i = tid; i < NB; i += kThreads) lh[i] = 0;
        __syncthreads();
        stream(R.lg, a.lgs[2], R.lo, R.hi, [&](uint32_t im) {
            if ((im & mask) == prefix) atomicAdd(&lh[(im >> SH) & (uint32_t)(NB - 1)], 1);
        });
        __syncthreads();
        for (int i = tid; i < NB; i += kThreads) {
            const int v = lh[i];
            if (v) atomicAdd(&h[doff(P) + i], v);
        }
    } else {
        int gt = 0, eq = 0;
        stream(R.lg, a.lgs[2], R.lo, R.hi, [&](uint32_t im) {
            gt += im > prefix;
            eq += im == prefix;
        });
        gt = wave_sum_to_lane0(gt);
        eq = wave_sum_to_lane0(eq);
        if ((tid & 63) == 0) {
            lh[tid >> 6] = gt;
            lh[kWaves + (tid >> 6)] = eq;
        }
        __syncthreads();
        if (tid == 0) {
            int2 c{0, 0};
#pragma unroll
            for (int k = 0; k < kWaves; ++k) {
                c.x += lh[k];
                c.y += lh[kWaves + k];
            }
            reinterpret_cast<int2 *>(w.cnt)[(int64_t)R.r * w.splits + blockIdx.x] = c;
        }
    }
}

template <bool VQ> __global__ __launch_bounds__(kThreads) void fa2_topk_split_emit_kernel(const Fa2IndexerProblem a, const SplitArgs w) {
    __shared__ Scan S;
    __shared__ int wsum[kWaves];
    __shared__ int s_base[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Row R;
    if (!split_row<VQ>(a, w, R)) return;
    int32_t *out = R.out;
    if (R.n <= a.topk) {  // the identity prefix, no logit read
        if (blockIdx.x == 0)
            for (int s = tid; s < a.topk; s += kThreads) out[(int64_t)s * a.is[2]] = s < R.n ? s : -1;
        return;
    }
    if (R.lo >= R.n) return;
    uint32_t T;
    int take;  // >= 1
    derive<3>(w.hist + (int64_t)R.r * kTopkBins, a.topk, S, T, take);
    if (wave == 0) {  // the candidates above T and equal to T in the splits before this one
        const int2 *c = reinterpret_cast<const int2 *>(w.cnt) + (int64_t)R.r * w.splits;
        int g = 0, e = 0;
        for (int k = lane; k < (int)blockIdx.x; k += 64) {
            g += c[k].x;
            e += c[k].y;
        }
        g = wave_sum_to_lane0(g);
        e = wave_sum_to_lane0(e);
        if (lane == 0) {
            s_base[0] = g;
            s_base[1] = e;
        }
    }
    __syncthreads();
    int base_gt = s_base[0], base_eq = s_base[1];

    // the ordered compaction of fa2_indexer_topk.hip over [lo, hi)
    const float *lg = R.lg;
    const int n = R.hi;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int j0 = R.lo; j0 < n; j0 += kThreads) {  // (the same trip count for every thread: barriers inside)
        const int j = j0 + tid;
        const uint32_t im = j < n ? image(lg[(int64_t)j * a.lgs[2]]) : 0u;
        const bool gt = j < n && im > T, eq = j < n && im == T;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        if (lane == 0) wsum[wave] = __popcll(bg) | (__popcll(be) << 16);  // (each <= 64)
        __syncthreads();
        int og = 0, oe = 0, tg = 0, te = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const int v = wsum[k], vg = v & 0xffff, ve = v >> 16;
            if (k < wave) {
                og += vg;
                oe += ve;
            }
            tg += vg;
            te += ve;
        }
        const int gt_before = base_gt + og + __popcll(bg & below), eq_before = base_eq + oe + __popcll(be & below);
        const int slot = gt_before + (eq_before < take ? eq_before : take);
        if ((gt || (eq && eq_before < take)) && slot < a.topk) out[(int64_t)slot * a.is[2]] = j;
        base_gt += tg;
        base_eq += te;
        __syncthreads();
    }
}

}  // namespace

#if FA2_INDEXER_VARLEN
int fa2_launch_topk_indices_split_v(const Fa2IndexerProblem &p, int splits, int chunk, void *workspace) {
#else
int fa2_launch_topk_indices_split(const Fa2IndexerProblem &p, int splits, int chunk, void *workspace) {
#endif
    const long long rows = kVQ ? (long long)p.total_q : (long long)p.B * p.N_q;
    if (rows > 65535 || splits < 2 || splits > kTopkMaxSplits || chunk < kThreads) {
        fa2_set_error("topk indices split: grid too large or no split (rows = %lld, num_splits = %d, chunk = %d)", rows, splits, chunk);
        return FA2_ERR_BAD_ARG;
    }
    SplitArgs w{(int32_t *)workspace, (int32_t *)workspace + rows * kTopkBins, splits, chunk};
    const dim3 grid((unsigned)splits, (unsigned)rows), block(kThreads);
    hipLaunchKernelGGL(fa2_topk_split_zero_kernel, dim3(kTopkBins / (4 * 256), (unsigned)rows), dim3(256), 0, p.stream, (int4 *)workspace);
    hipLaunchKernelGGL((fa2_topk_split_pass_kernel<kVQ, 0>), grid, block, 0, p.stream, p, w);
    hipLaunchKernelGGL((fa2_topk_split_pass_kernel<kVQ, 1>), grid, block, 0, p.stream, p, w);
    hipLaunchKernelGGL((fa2_topk_split_pass_kernel<kVQ, 2>), grid, block, 0, p.stream, p, w);
    hipLaunchKernelGGL((fa2_topk_split_pass_kernel<kVQ, 3>), grid, block, 0, p.stream, p, w);
    hipLaunchKernelGGL(fa2_topk_split_emit_kernel<kVQ>, grid, block, 0, p.stream, p, w);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("topk indices split kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}
