// fa2_indexer_mfma8.hip -- the index scores of the MLA indexer with fp8 QUERIES on the fp8 matrix cores (fa2_mla_indexer_logits_q8,
// FA2_INDEXER_VARIANT_IDX8): q_idx and the index-key cache each in e4m3fn or e5m2 (the two need not match), d_I = 128, H_I <= 64.
//
//     logit[b, qi, j] = k_scale[b, j] * sum_h w[b, h, qi] * max(0, q8[b, h, qi, :] . k8[b, j, :])
//
// There is no q_scale: the caller has folded the queries' scale into w.  With d_I = 128 ONE v_mfma_f32_16x16x128_f8f6f4 is the whole
// dot product of 16 heads against 16 keys: no accumulation chain (every MFMA starts from zero), no conversion while staging, half
// the LDS bytes per tile and half the registers per Q fragment of the 16-bit form (fa2_indexer_mfma16.hip).  That is what this
// kernel's split is built on; the grid, the causal skipping and the packed rows are that file's.
//
// Work.  One workgroup of four waves owns kIdx8QB = 16 consecutive query positions of one sequence and one chunk of its keys; the
// grid is (key chunks * query blocks, B), the query block running fastest.  The tile is 64 heads of one position against 64 keys,
// heads as the rows: D[head 4g + r][key n] for lane (n = lane & 15, g = lane >> 4).  The waves split the HEADS: wave w holds the A
// fragments of heads 16w .. 16w + 15 for all sixteen positions -- 8 registers a position, 128 in all -- and runs 4 MFMAs per position
// and tile, one per 16-key block.  The k index of an MFMA is only a summation index: lane (n, g) feeds bytes 32g .. 32g + 31 of its row
// to A and B alike.  Heads at and past H_I are zero rows with weight 0.  The weights live in LDS ([16][64] fp32, 4 KiB; a lane reads
// the four of its accumulator rows in one 16-byte read), which keeps the wave under 256 registers: two waves per SIMD, so one wave's
// MFMAs run under the other's VALU epilogue.
//
// Staging.  The bytes go to LDS as they are: an 8 KiB [64][128 B] tile under the 128-byte-row swizzle of fa2_mfma.h (lds_off<64>),
// 16-byte loads into registers a step ahead (two per thread and tile), DOUBLE-BUFFERED, and the waves' shares double-buffered too,
// so a tile costs ONE barrier: step t computes on tile buffer t & 1 into share buffer t & 1, writes tile t + 1 into the other
// buffer (last read before the previous barrier), meets the barrier, then sums and stores from share buffer t & 1 (next written two
// barriers on).  Rows at and past the block's bound are not loaded (zeros in LDS): nothing behind cache_seqlens[b] is read.
// Paged cache: the staging thread looks its own row up, the table entry clamped, ANY page size.
//
// Epilogue.  Per position and tile: ReLU, times w[h], the sum over the four accumulator rows, for each of the four key blocks; then
// the sum over g as a reduce-scatter over all four blocks at once -- v_permlane16_swap on the pairs (0, 1) and (2, 3), one add each,
// then v_permlane32_swap on the two sums and one add: three exchanges where the 16-bit form spends eight -- which leaves lane (n, g)
// the wave's share of key 16g + n.  After the barrier thread (position, key) adds the four waves' shares IN WAVE ORDER (a result
// does not depend on the launch), multiplies by k_scale[j] and stores 64 consecutive fp32 per position.  A position whose bound
// lies at or below the tile's first key skips the tile; keys at and past a position's bound are not stored.
//
// Packed queries (fa2_mla_indexer_logits_varlen_q8): VQ, instantiated in fa2_indexer_mfma8_v.hip (FA2_INDEXER_VARLEN) alone, exactly as
// in fa2_indexer_mfma16.hip: the block takes its sequence's rows from cu_q, leaves before any barrier when it has no position, and a
// query block never crosses a sequence.
#include "fa2_decode.h"
#include "fa2_indexer.h"
#include "fa2_mfma.h"

#ifndef FA2_INDEXER_VARLEN
#define FA2_INDEXER_VARLEN 0
#endif

namespace {

constexpr bool kVQ = FA2_INDEXER_VARLEN != 0;

struct Idx8Args {
    const char *Q, *K;
    const float *W, *KS;
    float *LG;
    int64_t qs[3];  // B, H, N strides (bytes = elements; column stride 1)
    int64_t ws[3];
    int64_t ks[2];  // batch (or block) and row strides
    int64_t kss[2], lgs[3];
    const int32_t *seqlens, *table;
    int64_t table_stride;
    int page_size, num_blocks;
    int H, N_q, S_k, causal;
    int chunk, nqb;  // keys per workgroup (a multiple of 64), query blocks per sequence
    const int32_t *cu_q;  // VQ only: B + 1 offsets into the packed rows; qs[0] = ws[0] = lgs[0] = 0, N_q holds max_seqlen_q
    int total_q;
};

constexpr int kTileKeys = 64;
constexpr int kRowB = 128;                     // an fp8 LDS row of 128 columns
constexpr int kTileB = kTileKeys * kRowB;      // 8 KiB, two of them
constexpr int kPartB = kIdx8QB * 4 * 64 * 4;   // [position][wave][key] fp32 shares: 16 KiB, two of them
constexpr int kWB = kIdx8QB * 64 * 4;          // [position][head] fp32 weights

// The sum over g of four per-lane values, block kb's left on the lanes of g = kb.  v_permlane16_swap(a, b) swaps the odd 16-lane rows
// of a with the even rows of b: a' = [a0 b0 a2 b2], b' = [a1 b1 a3 b3] (rows by g), so a' + b' is (v0[g] + v0[g ^ 1]) on even g and
// (v1[g] + v1[g ^ 1]) on odd g; v_permlane32_swap does the same with the wave's halves.  (The elements are copied to scalars before
// the bit cast: fa2_mfma.h, half_swap.)
__device__ __forceinline__ float swap16_sum(float x, float y) {
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), false, false);
    const unsigned a = r[0], b = r[1];
    return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float swap32_sum(float x, float y) {
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, x), __builtin_bit_cast(unsigned, y), false, false);
    const unsigned a = r[0], b = r[1];
    return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}

// FQ, FK: the formats of q_idx and k_idx (0 = e4m3, 1 = e5m2).  Two waves per SIMD: at most 256 unified registers.
template <int FQ, int FK, bool PAGED, bool VQ>
__global__ __launch_bounds__(256, 2) void fa2_indexer_mfma8_kernel(const Idx8Args a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kTileB + 2 * kPartB + kWB];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;
    LDS_PTR(float) part = (LDS_PTR(float))(lds + 2 * kTileB);
    LDS_PTR(float) wl = (LDS_PTR(float))(lds + 2 * kTileB + 2 * kPartB);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    unsigned bx = blockIdx.x;
    if constexpr (VQ) {
        // Sequence b takes its blocks rotated by b: with query block 0 of every key chunk nqb ids apart, the live blocks of one-token
        // sequences would all land on ONE XCD where nqb is a multiple of their number (fa2_indexer_mfma16.hip has the measurement).  A
        // bijection of the same grid.
        bx += blockIdx.y % gridDim.x;  // (< 2^31 + 2^16: inside an unsigned)
        bx -= bx >= gridDim.x ? gridDim.x : 0;
    }
    const int ck = (int)bx / a.nqb, q0 = ((int)bx - ck * a.nqb) * kIdx8QB;

    // N_q: the query count of the sequence, from packed row `start` on
    int N_q = a.N_q, start = 0;
    if constexpr (VQ) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.N_q, start, N_q);
        if (q0 >= N_q) return;  // no position of this block (uniform: before any barrier)
    }
    // the candidate counts of the block's positions (fa2_indexer_count; 0 for a position past N_q), non-decreasing: the last live
    // position's is the block's bound.  Recomputed from three uniform values where they are used: sixteen kept counts cost the kernel
    // its scalar registers.
    int nk = a.seqlens ? a.seqlens[b] : a.S_k;
    nk = nk < 0 ? 0 : (nk > a.S_k ? a.S_k : nk);
    const int nlive = N_q - q0, cbase = nk - N_q + q0 + 1;  // causal: position p has min(cbase + p, nk) candidates, none below 1
    auto cnt = [&](int p) -> int {
        if (p >= nlive) return 0;
        if (!a.causal) return nk;
        const int c = cbase + p;
        return c < 0 ? 0 : (c < nk ? c : nk);
    };
    const int bound = cnt(nlive < kIdx8QB ? nlive - 1 : kIdx8QB - 1);
    const int k0 = ck * a.chunk;
    const int ke = k0 + a.chunk < bound ? k0 + a.chunk : bound;
    if (k0 >= ke) return;  // (uniform)
    const int nt = (ke - k0 + kTileKeys - 1) / kTileKeys;

    // ---- A fragments: lane (n, g) holds Q[head 16 wave + n][32 g .. 32 g + 31]
    i32x8 qf[kIdx8QB];
#pragma unroll
    for (int p = 0; p < kIdx8QB; ++p) {
        const int qi = q0 + p, head = 16 * wave + n;
        u32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (qi < N_q && head < a.H) {
            const char *qp = a.Q + b * a.qs[0] + (int64_t)head * a.qs[1] + (int64_t)(start + qi) * a.qs[2] + g * 32;
            lo = *(const u32x4 *)qp;
            hi = *(const u32x4 *)(qp + 16);
        }
        qf[p] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    }
    // ---- the weights: wl[position][head], 0 for a head at or past H_I and a position at or past N_q
#pragma unroll
    for (int i = 0; i < kWB / 4 / 256; ++i) {
        const int e = tid + 256 * i, p = e >> 6, hh = e & 63, qi = q0 + p;
        wl[e] = qi < N_q && hh < a.H ? a.W[b * a.ws[0] + hh * a.ws[1] + (start + qi) * a.ws[2]] : 0.0f;
    }

    // ---- staging map: thread handles chunk (row = 32 it + tid / 8, ch = tid % 8) of each tile
    const int st_row = tid >> 3, st_ch = tid & 7;
    const int st_lds = lds_off<64>(st_row, st_ch);  // (the swizzle is a function of row & 15: a pass covers 32 rows)
    const int32_t *tab = PAGED ? a.table + b * a.table_stride : nullptr;
    // key j < ke <= N_k(b) <= capacity: its page index is below max_blocks
    auto key_row = [&](int j, int64_t s0, int64_t s1) -> int64_t {
        if constexpr (PAGED) {
            const int pg = j / a.page_size;
            return fa2_decode_page(tab, pg, a.num_blocks) * s0 + (int64_t)(j - pg * a.page_size) * s1;
        } else {
            return b * s0 + (int64_t)j * s1;
        }
    };
    u32x4 kreg[2];
    auto stage_load = [&](int t) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int j = k0 + t * kTileKeys + it * 32 + st_row;
            kreg[it] = j < ke ? *(const u32x4 *)(a.K + key_row(j, a.ks[0], a.ks[1]) + st_ch * 16) : u32x4{0, 0, 0, 0};
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int it = 0; it < 2; ++it) *(LDS_PTR(u32x4))(lds + buf * kTileB + st_lds + it * 32 * kRowB) = kreg[it];
    };

    // ---- B fragments: lane (n, g) reads chunks 2 g, 2 g + 1 of K row 16 kb + n
    const int k_off0 = lds_off<64>(n, 2 * g), k_off1 = lds_off<64>(n, 2 * g + 1);
    const int w_off = 16 * wave + 4 * g;  // the heads of this lane's accumulator rows

    stage_load(0);
    stage_write(0);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const bool more = t + 1 < nt;
        const int cur = t & 1;
        if (more) stage_load(t + 1);
        const int tk0 = k0 + t * kTileKeys;

        i32x8 kf[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const u32x4 lo = *(LDS_PTR(u32x4))(lds + cur * kTileB + kb * 16 * kRowB + k_off0);
            const u32x4 hi = *(LDS_PTR(u32x4))(lds + cur * kTileB + kb * 16 * kRowB + k_off1);
            kf[kb] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        }

        LDS_PTR(float) pt = part + cur * (kPartB / 4);
#pragma unroll
        for (int p = 0; p < kIdx8QB; ++p) {
            if (tk0 >= cnt(p)) continue;  // (uniform) the tile lies wholly past this position's bound
            const f32x4 w4 = *(LDS_PTR(f32x4))(wl + p * 64 + w_off);
            float v[4];
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const f32x4 acc = mfma_f8_16x16x128<FQ, FK>(qf[p], kf[kb], f32x4{0.0f, 0.0f, 0.0f, 0.0f});
                float s = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) s += w4[r] * fmaxf(acc[r], 0.0f);
                v[kb] = s;
            }
            // block g & 1 of (0, 1) and block 2 + (g & 1) of (2, 3) summed over g ^ 1; then block g summed over all four g
            pt[(p * 4 + wave) * 64 + lane] = swap32_sum(swap16_sum(v[0], v[1]), swap16_sum(v[2], v[3]));
        }
        if (more) stage_write(cur ^ 1);
        __syncthreads();  // the shares and the next tile are visible; every read of this tile has retired

        const int j = tk0 + lane;
        float ksc = 1.0f;
        if (j < ke) ksc = a.KS[key_row(j, a.kss[0], a.kss[1])];
#pragma unroll
        for (int p = 0; p < kIdx8QB; ++p) {
            if ((p & 3) != wave || j >= cnt(p)) continue;
            const float s = ((pt[(p * 4 + 0) * 64 + lane] + pt[(p * 4 + 1) * 64 + lane]) + pt[(p * 4 + 2) * 64 + lane]) +
                            pt[(p * 4 + 3) * 64 + lane];
            a.LG[b * a.lgs[0] + (int64_t)(start + q0 + p) * a.lgs[1] + (int64_t)j * a.lgs[2]] = s * ksc;
        }
    }
}

template <int FQ, int FK, bool PAGED> int launch_t(const Fa2IndexerProblem &p, const Idx8Args &a) {
    const long long gx = (long long)a.nqb * ((p.S_k + a.chunk - 1) / a.chunk);
    if (gx > 0x7fffffffLL) {
        fa2_set_error("mla indexer: grid too large (query blocks * key chunks = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL((fa2_indexer_mfma8_kernel<FQ, FK, PAGED, kVQ>), dim3((unsigned)gx, p.B), dim3(256), 0, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("mla indexer idx8 kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <int FQ, int FK> int launch_p(const Fa2IndexerProblem &p, const Idx8Args &a) {
    return p.table ? launch_t<FQ, FK, true>(p, a) : launch_t<FQ, FK, false>(p, a);
}

template <int FQ> int launch_k(const Fa2IndexerProblem &p, const Idx8Args &a) {
    return p.k_dtype == FA2_DTYPE_F8E4M3 ? launch_p<FQ, 0>(p, a) : launch_p<FQ, 1>(p, a);
}

bool fp8(int32_t dt) { return dt == FA2_DTYPE_F8E4M3 || dt == FA2_DTYPE_F8E5M2; }

bool supports(const Fa2IndexerProblem &p) {
    if ((p.cu_q != nullptr) != kVQ) return false;
    if (!fp8(p.dtype) || !fp8(p.k_dtype) || !p.KS) return false;
    if (p.d != 128 || p.H > 64) return false;
    if (p.qs[3] != 1 || p.ks[2] != 1) return false;
    // 16-byte vector loads of the Q and K rows: every row start must stay aligned (16 elements)
    for (int k = 0; k < 3; ++k)
        if (p.qs[k] & 15) return false;
    if ((p.ks[0] & 15) || (p.ks[1] & 15)) return false;
    if (((uintptr_t)p.Q & 15) || ((uintptr_t)p.K & 15)) return false;
    return true;
}

int launch(const Fa2IndexerProblem &p) {
    if (!supports(p)) {
        fa2_set_error("mla indexer idx8 kernel: needs fp8 q_idx and k_idx, d_I = 128, H_I <= 64, unit column strides, 16-byte aligned "
                      "rows");
        return FA2_ERR_UNSUPPORTED;
    }
    Idx8Args a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K; a.W = p.W; a.KS = p.KS; a.LG = p.LG;
    for (int k = 0; k < 3; ++k) { a.qs[k] = p.qs[k]; a.ws[k] = p.ws[k]; a.lgs[k] = p.lgs[k]; }
    for (int k = 0; k < 2; ++k) { a.ks[k] = p.ks[k]; a.kss[k] = p.kss[k]; }
    a.seqlens = p.seqlens; a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.H = p.H; a.N_q = p.N_q; a.S_k = p.S_k; a.causal = p.causal;
    // The two regimes of the 16-bit form (fa2_indexer_mfma16.hip): 256-key chunks while there are fewer than 256 (sequence, query
    // block) pairs -- a decode step wants the chip full -- and 2,048 from there on.  (packed: the query blocks that have positions are at
    // most the grid's, and at most ceil(total_q / 16) + B)
    a.nqb = (p.N_q + kIdx8QB - 1) / kIdx8QB;
    long long blocks = (long long)p.B * a.nqb;
    if (kVQ && (p.total_q + kIdx8QB - 1) / kIdx8QB + (long long)p.B < blocks) blocks = (p.total_q + kIdx8QB - 1) / kIdx8QB + (long long)p.B;
    a.chunk = blocks >= 256 ? 2048 : 256;
    a.cu_q = p.cu_q; a.total_q = p.total_q;
    return p.dtype == FA2_DTYPE_F8E4M3 ? launch_k<0>(p, a) : launch_k<1>(p, a);
}

}  // namespace

#if FA2_INDEXER_VARLEN
bool fa2_indexer_mfma8_v_supports(const Fa2IndexerProblem &p) { return supports(p); }
int fa2_launch_indexer_mfma8_v(const Fa2IndexerProblem &p) { return launch(p); }
#else
bool fa2_indexer_mfma8_supports(const Fa2IndexerProblem &p) { return supports(p); }
int fa2_launch_indexer_mfma8(const Fa2IndexerProblem &p) { return launch(p); }
#endif
