// fa2_indexer_mfma16.hip -- the index scores of the MLA indexer on the matrix cores (fa2_mla_indexer_logits,
// FA2_INDEXER_VARIANT_IDX16): f16 / bf16 q_idx, the index-key cache alike or fp8 storage, d_I = 128, H_I <= 64.
//
//     logit[b, qi, j] = k_scale[b, j] * sum_h w[b, h, qi] * max(0, q[b, h, qi, :] . k[b, j, :])
//
// One workgroup of four waves owns kIdxQB = 8 consecutive query positions of one sequence and one chunk of its keys; the grid is
// (key chunks * query blocks, B), the query block running fastest, so neighbours read the same keys.  The tile is 64 heads of one
// position against 64 keys on v_mfma_f32_16x16x32, heads as the rows: D[head 4g + r][key n] = Q (A, registers) . K^T (B, LDS) for
// lane (n = lane & 15, g = lane >> 4).  The waves split the HEADS: wave w holds the A fragments of heads 16w .. 16w + 15 for all
// eight positions (16 registers a position) and the weights of its four accumulator rows; heads at and past H_I are zero rows with
// weight 0.  There is no softmax and no state across tiles.
//
// Per step the workgroup takes ONE 64-key tile, staged once (16-byte loads into registers a step ahead, then the swizzled [64][128]
// 16-bit LDS image of fa2_mfma.h; an fp8 row is converted exactly on the way, CacheCvt).  Every wave reads the tile's 16 B fragments
// once and runs all its positions against them: 16 MFMAs a position, then ReLU, the weights, the sum over the four accumulator rows
// and two lane exchanges (the sum over g), which leaves the wave's share of 64 logits, one per lane, in LDS.  After a barrier
// thread (position, key) adds the four waves' shares in wave order, multiplies by k_scale[j] and stores: 64 consecutive fp32 per
// position.  A position whose causal bound lies at or below the tile's first key skips the tile; a tile wholly past the bound of
// the block's last position ends the chunk; keys at and past a position's bound are not stored, and rows at and past the block's
// bound are not loaded (zeros in LDS), so what lies behind cache_seqlens[b] is never read.
//
// Paged cache: key j is row j % page_size of page table[b][j / page_size] for ANY page size -- the staging thread looks its own
// row up (one division and one clamped table entry per 16-byte load), so no page size falls to the VALU form.
//
// Packed queries (fa2_mla_indexer_logits_varlen).  VQ is a template parameter, instantiated in fa2_indexer_mfma16_v.hip
// (FA2_INDEXER_VARLEN) alone.  The grid is (key chunks * ceil(max_seqlen_q / 8), B): the block takes its sequence's start and
// n_q(b) from cu_q (fa2_varlen_seq), leaves at once -- uniform, before any barrier -- when its first position is at or past n_q(b),
// counts the candidates with n_q(b) in N_q's place, and reads Q, W and writes the logits at packed row start + position (no batch
// stride).  A query block never crosses a sequence.  Everything else is the fixed form's.
#include "fa2_decode.h"
#include "fa2_indexer.h"
#include "fa2_mfma.h"

#ifndef FA2_INDEXER_VARLEN
#define FA2_INDEXER_VARLEN 0
#endif

namespace {

constexpr bool kVQ = FA2_INDEXER_VARLEN != 0;

struct Idx16Args {
    const char *Q, *K;
    const float *W, *KS;
    float *LG;
    int64_t qs[3];  // B, H, N strides in BYTES (column stride 1 element)
    int64_t ws[3];
    int64_t ks[2];  // batch (or block) and row strides in BYTES
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
constexpr int kRowB = 256;                     // a 16-bit LDS row of 128 columns
constexpr int kTileB = kTileKeys * kRowB;      // 16 KiB
constexpr int kPartB = kIdxQB * 4 * 64 * 4;    // [position][wave][key] fp32 shares

template <typename T, typename C, bool PAGED, bool VQ>
__global__ __launch_bounds__(256) void fa2_indexer_mfma16_kernel(const Idx16Args a) {
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr bool F8 = !__is_same(C, T);
    constexpr int GROWB = F8 ? 128 : 256;                  // bytes of a cache row in memory
    constexpr int CPR = GROWB / 16, RPI = 256 / CPR, CPT = kTileKeys / RPI;  // 16-byte loads per row; rows per pass; passes
    __shared__ __attribute__((aligned(16))) char smem[kTileB + kPartB];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;
    LDS_PTR(float) part = (LDS_PTR(float))(lds + kTileB);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    unsigned bx = blockIdx.x;
    if constexpr (VQ) {
        // The hardware deals consecutive workgroup ids round the chip's XCDs.  With query block 0 of every key chunk at x = chunk *
        // nqb, the blocks of a one-token sequence that have a position sit nqb ids apart, and where nqb is a multiple of the number
        // of XCDs they all land on ONE of them (measured: a 256-token chunk beside 63 one-token decodes, nqb = 32, took 2,596 us in
        // the indexer against 300 us for the two fixed calls).  So sequence b takes its blocks rotated by b, as the query-tiled
        // latent kernel does (fa2_decode_mla16.hip): the blocks of a chunk stay neighbours, the live blocks of consecutive
        // sequences sit on consecutive ids.  A bijection of the same grid.
        bx += blockIdx.y % gridDim.x;  // (< 2^31 + 2^16: inside an unsigned)
        bx -= bx >= gridDim.x ? gridDim.x : 0;
    }
    const int ck = (int)bx / a.nqb, q0 = ((int)bx - ck * a.nqb) * kIdxQB;

    // N_q: the query count of the sequence, from packed row `start` on
    int N_q = a.N_q, start = 0;
    if constexpr (VQ) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.N_q, start, N_q);
        if (q0 >= N_q) return;  // no position of this block (uniform: before any barrier)
    }
    // the candidate counts of the block's positions (0 for a position past N_q), non-decreasing: the last is the block's bound
    int cnt[kIdxQB];
    int bound = 0;
#pragma unroll
    for (int p = 0; p < kIdxQB; ++p) {
        cnt[p] = q0 + p < N_q ? fa2_indexer_count(a.seqlens, b, a.S_k, N_q, q0 + p, a.causal) : 0;
        bound = cnt[p] > bound ? cnt[p] : bound;
    }
    const int k0 = ck * a.chunk;
    const int ke = k0 + a.chunk < bound ? k0 + a.chunk : bound;
    if (k0 >= ke) return;  // (uniform)
    const int nt = (ke - k0 + kTileKeys - 1) / kTileKeys;

    // ---- A fragments: lane (n, g) holds Q[head 16 wave + n][32 ks + 8 g .. + 7]; and the weights of accumulator rows 4 g + r
    frag qf[kIdxQB][4];
    float wv[kIdxQB][4];
#pragma unroll
    for (int p = 0; p < kIdxQB; ++p) {
        const int qi = q0 + p;
        const bool live = qi < N_q;
        const int head = 16 * wave + n;
        const char *qp = a.Q + b * a.qs[0] + (int64_t)head * a.qs[1] + (int64_t)(start + qi) * a.qs[2] + g * 16;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            qf[p][ks] = __builtin_bit_cast(frag, live && head < a.H ? *(const u32x4 *)(qp + ks * 64) : u32x4{0, 0, 0, 0});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int hh = 16 * wave + 4 * g + r;
            wv[p][r] = live && hh < a.H ? a.W[b * a.ws[0] + hh * a.ws[1] + (start + qi) * a.ws[2]] : 0.0f;
        }
    }

    // ---- staging map: thread handles chunk (row = it * RPI + tid / CPR, ch = tid % CPR) of each tile
    const int st_row = tid / CPR, st_ch = tid % CPR;
    const int st_lds = lds_off<128>(st_row, F8 ? 2 * st_ch : st_ch);
    const int st_lds1 = F8 ? lds_off<128>(st_row, 2 * st_ch + 1) : 0;
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
    u32x4 kreg[CPT];
    auto stage_load = [&](int t) {
#pragma unroll
        for (int it = 0; it < CPT; ++it) {
            const int j = k0 + t * kTileKeys + it * RPI + st_row;
            kreg[it] = j < ke ? *(const u32x4 *)(a.K + key_row(j, a.ks[0], a.ks[1]) + st_ch * 16) : u32x4{0, 0, 0, 0};
        }
    };
    auto stage_write = [&]() {
#pragma unroll
        for (int it = 0; it < CPT; ++it) {
            if constexpr (F8) {  // word j of the load = elements 4j .. 4j + 3 = words 2j, 2j + 1 of the 16-bit row
                using X = CacheCvt<T, C>;
                const u32x4 w = kreg[it];
                const u32x4 lo = {X::template cvt<false>(w[0]), X::template cvt<true>(w[0]), X::template cvt<false>(w[1]),
                                  X::template cvt<true>(w[1])};
                const u32x4 hi = {X::template cvt<false>(w[2]), X::template cvt<true>(w[2]), X::template cvt<false>(w[3]),
                                  X::template cvt<true>(w[3])};
                *(LDS_PTR(u32x4))(lds + st_lds + it * RPI * kRowB) = lo;
                *(LDS_PTR(u32x4))(lds + st_lds1 + it * RPI * kRowB) = hi;
            } else {
                *(LDS_PTR(u32x4))(lds + st_lds + it * RPI * kRowB) = kreg[it];
            }
        }
    };
    static_assert(RPI % 16 == 0, "the swizzle is a function of row & 15: a staging pass must cover a multiple of 16 rows");

    // ---- B fragments: lane (n, g) reads K row 16 kb + n, chunk 4 ks + g
    int k_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) k_off[ks] = lds_off<128>(n, 4 * ks + g);

    stage_load(0);
    stage_write();
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const bool more = t + 1 < nt;
        if (more) stage_load(t + 1);
        const int tk0 = k0 + t * kTileKeys;

        frag kf[4][4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                kf[kb][ks] = __builtin_bit_cast(frag, *(LDS_PTR(u32x4))(lds + kb * 16 * kRowB + k_off[ks]));

#pragma unroll
        for (int p = 0; p < kIdxQB; ++p) {
            if (tk0 >= cnt[p]) continue;  // (uniform) the tile lies wholly past this position's bound
            float share = 0.0f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) acc = M::mfma16(qf[p][ks], kf[kb][ks], acc);
                float v = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) v += wv[p][r] * fmaxf(acc[r], 0.0f);
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (g == kb) share = v;  // key 16 kb + n = this lane's index
            }
            part[(p * 4 + wave) * 64 + lane] = share;
        }
        __syncthreads();  // every read of the tile has retired; the shares are visible

        {
            const int j = tk0 + lane;
            float ksc = 1.0f;
            if (a.KS && j < ke) ksc = a.KS[key_row(j, a.kss[0], a.kss[1])];
#pragma unroll
            for (int p = 0; p < kIdxQB; ++p) {
                if ((p & 3) != wave || j >= cnt[p]) continue;
                const float s = ((part[(p * 4 + 0) * 64 + lane] + part[(p * 4 + 1) * 64 + lane]) + part[(p * 4 + 2) * 64 + lane]) +
                                part[(p * 4 + 3) * 64 + lane];
                a.LG[b * a.lgs[0] + (int64_t)(start + q0 + p) * a.lgs[1] + (int64_t)j * a.lgs[2]] = s * ksc;
            }
        }
        if (more) stage_write();
        __syncthreads();
    }
}

template <typename T, typename C, bool PAGED> int launch_t(const Fa2IndexerProblem &p, const Idx16Args &a) {
    const long long gx = (long long)a.nqb * ((p.S_k + a.chunk - 1) / a.chunk);
    if (gx > 0x7fffffffLL) {
        fa2_set_error("mla indexer: grid too large (query blocks * key chunks = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL((fa2_indexer_mfma16_kernel<T, C, PAGED, kVQ>), dim3((unsigned)gx, p.B), dim3(256), 0, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("mla indexer idx16 kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <typename T, typename C> int launch_p(const Fa2IndexerProblem &p, const Idx16Args &a) {
    return p.table ? launch_t<T, C, true>(p, a) : launch_t<T, C, false>(p, a);
}

template <typename T> int launch_c(const Fa2IndexerProblem &p, const Idx16Args &a) {
    if (p.k_dtype == FA2_DTYPE_F8E4M3) return launch_p<T, CacheE4M3>(p, a);
    if (p.k_dtype == FA2_DTYPE_F8E5M2) return launch_p<T, CacheE5M2>(p, a);
    return launch_p<T, T>(p, a);
}

bool fp8_cache(const Fa2IndexerProblem &p) { return p.k_dtype == FA2_DTYPE_F8E4M3 || p.k_dtype == FA2_DTYPE_F8E5M2; }

bool supports(const Fa2IndexerProblem &p) {
    if ((p.cu_q != nullptr) != kVQ) return false;
    if (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16) return false;
    if (p.k_dtype != p.dtype && !fp8_cache(p)) return false;
    if (p.d != 128 || p.H > 64) return false;
    if (p.qs[3] != 1 || p.ks[2] != 1) return false;
    // 16-byte vector loads of the Q and K rows: every row start must stay aligned (an fp8 cache: 16 elements)
    const int64_t kmask = fp8_cache(p) ? 15 : 7;
    for (int k = 0; k < 3; ++k)
        if (p.qs[k] & 7) return false;
    if ((p.ks[0] & kmask) || (p.ks[1] & kmask)) return false;
    if (((uintptr_t)p.Q & 15) || ((uintptr_t)p.K & 15)) return false;
    return true;
}

int launch(const Fa2IndexerProblem &p) {
    if (!supports(p)) {
        fa2_set_error("mla indexer idx16 kernel: needs f16/bf16 q_idx (the cache alike, or fp8), d_I = 128, H_I <= 64, unit column "
                      "strides, 16-byte aligned rows");
        return FA2_ERR_UNSUPPORTED;
    }
    Idx16Args a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K; a.W = p.W; a.KS = p.KS; a.LG = p.LG;
    const int64_t cb = fp8_cache(p) ? 1 : 2;  // bytes per cache element
    for (int k = 0; k < 3; ++k) { a.qs[k] = p.qs[k] * 2; a.ws[k] = p.ws[k]; a.lgs[k] = p.lgs[k]; }
    for (int k = 0; k < 2; ++k) { a.ks[k] = p.ks[k] * cb; a.kss[k] = p.kss[k]; }
    a.seqlens = p.seqlens; a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.H = p.H; a.N_q = p.N_q; a.S_k = p.S_k; a.causal = p.causal;
    // The two regimes.  A decode step (one or two positions: one query block a sequence) is bound by the read of the cache and wants
    // the chip full: 256-key chunks, four tiles a workgroup.  A prefill chunk (hundreds of query blocks) is bound by the matrix
    // work; its workgroups are many already, and a 2,048-key chunk re-reads the 128 KiB of a block's Q fragments once per 32 tiles.
    // (packed: the query blocks that have positions are at most the grid's, and at most ceil(total_q / 8) + B)
    a.nqb = (p.N_q + kIdxQB - 1) / kIdxQB;
    long long blocks = (long long)p.B * a.nqb;
    if (kVQ && (p.total_q + kIdxQB - 1) / kIdxQB + (long long)p.B < blocks) blocks = (p.total_q + kIdxQB - 1) / kIdxQB + (long long)p.B;
    a.chunk = blocks >= 256 ? 2048 : 256;
    a.cu_q = p.cu_q; a.total_q = p.total_q;
    return p.dtype == FA2_DTYPE_BF16 ? launch_c<__bf16>(p, a) : launch_c<_Float16>(p, a);
}

}  // namespace

#if FA2_INDEXER_VARLEN
bool fa2_indexer_mfma16_v_supports(const Fa2IndexerProblem &p) { return supports(p); }
int fa2_launch_indexer_mfma16_v(const Fa2IndexerProblem &p) { return launch(p); }
#else
bool fa2_indexer_mfma16_supports(const Fa2IndexerProblem &p) { return supports(p); }
int fa2_launch_indexer_mfma16(const Fa2IndexerProblem &p) { return launch(p); }
#endif
