// fa2_decode_mla8.hip -- KV-cache decode over the fp8 latent cache with fp8 QUERIES (fa2_fwd_kvcache_mla_q8, FA2_KVCACHE_VARIANT_MLA8):
// multi-head latent attention in its absorbed form, e4m3fn on both sides, d = 576, d_v = 512, V = K[..., :512], the scores AND P.V on
// the fp8 matrix instruction v_mfma_f32_32x32x64_f8f6f4.  No byte of the cache is widened.
//
// Stated arithmetic.  With qd, kd, vd the descales at [b, h_kv] and c = scale log2(e) qd kd:
//     S  = c * sum_c q8[c] k8[c]        the products exact, the sum in fp32 on the matrix instruction (576 = 9 k-steps of 64)
//     p  = exp2(s - m) in fp32          online softmax in the exp2 domain, masked scores SELECTED to -inf; l adds the unrounded p
//     P8 = e4m3_rne(256 p)              the matrix operand: 256 keeps p down to 2^-14 in the normal range, 256 p <= 256 < 448
//     O  = vd 2^-8 (sum P8 v8) / l      fp32, rounded once to the output dtype -- or written as the normalised fp32 partial
//     L  = m + log2 l                   fp32
//
// Work split: fa2_decode_mla16.hip's.  One workgroup of four waves handles one (split, 64-row tile of a KV group, KV head, sequence),
// grid (num_splits * row_tiles, H_kv, B), row r = head-in-group * N_q + query, a last tile with fewer than 64 rows computing its
// padding rows (the last row again) and dropping them.
//
// The tile.  64 keys x 576 B go to LDS as they are, in rows of 640 B (40 16-byte chunks, 36 used): 40 KiB a tile, TWO tile buffers.
// Tile t + 1 is loaded (9 x 16 bytes a thread, in flight from the top of the step) and written to the other buffer while tile t is
// computed; a step has two barriers where the single-buffered 16-bit kernel has four.  A wave stages 16 rows = 576 loads = 9 passes
// under the flat index f = 64 pass + lane -> (row f / 36, chunk f % 36): consecutive lanes read consecutive 16-byte pieces and no load
// crosses a row.
//
// Banks.  Chunk ch of row r sits at r * 640 + ((ch ^ z(r)) << 4), z(r) = bit1(r) << 1 | bit3(r) << 2 | bit2(r): an XOR on the low three
// chunk bits (ch < 36 stays < 40).  640 B = 2.5 bank rows of 256 B, so the 16-byte slot of (r, ch) in its bank row is
// 8 ((r ^ ch >> 3) & 1) + ((ch & 7) ^ z(r)).
//   S phase:  a ds_read_b128 lane group reads ONE chunk of 16 consecutive rows; (r & 1, z(r)) is a bijection of r & 15, so the 16
//             reads fall into 16 different slots.
//   P.V:      a half-wave of ds_read_b64_tr_b8 reads, of the eight rows {0..3, 8..11} + 4 h of a 16-key step, the aligned chunk PAIR
//             (2 u, 2 u + 1), 32 B each.  The pair's 32-byte unit in the bank row is 4 ((r ^ u >> 2) & 1) + (((2 u & 7) ^ z(r)) >> 1),
//             and (r & 1, z(r) >> 1) = (bit0, bit1, bit3) separates exactly those eight rows (bit2 is 4 h's): eight different units.
//
//   S phase.   Wave w owns key block w & 1 and row block w >> 1 of S^T = K Q^T: 9 MFMAs, a lane (row i, half h) supplying per k-step s
//              the chunks 4 s + h and 4 s + 2 + h of its row (k is a summation index: Q is held with the same map, 72 registers,
//              resident).
//   Softmax.   The two key blocks of a row exchange their maxima through LDS.  A lane's 16 scores are keys 32 kb + (r & 3) + 8 (r >> 2)
//              + 4 h: packed to 16 bytes in register order they ARE k slots 16 kb .. + 15 of the P.V B fragment of lane (i, h) of
//              that row block -- one ds_write_b128, no lane exchange; P of the tile is 4 KiB at [kb][h][row], consecutive lanes
//              16 bytes apart for the write and for the reads.
//   P.V phase. Wave w owns value columns [128 w, 128 w + 128) for all 64 rows: ONE k-step of 64 keys per 32 x 32 block, 8 MFMAs a
//              step; the V^T fragment is four transposed reads (8 keys each, in the k-slot order above: the lane map of
//              fa2_mfma8x.hip) and feeds both row blocks.
//
// Stale cache contents: a key at or past the split's end (<= N_k(b)) is not loaded -- its LDS row is zeros and its score is selected
// to -inf -- so what lies behind cache_seqlens[b] is never read (a stale NaN byte under P8 = 0 would still poison the product).  Paged
// cache: page_size % 64 == 0, one scalar table entry per tile, clamped to [0, num_blocks - 1]; the entry of a tile at or past the
// split's end is not loaded.
//
// Output: num_splits == 1 writes O in the output dtype and L in fp32 (a row without a visible key: O = 0, L = +inf); otherwise every
// (split, row) writes the normalised fp32 partial (an empty split: 0 and -inf) for fa2_decode_combine.hip.  Vector stores only, no
// atomics, no hand-off between workgroups.
//
// Packed (ragged) queries (fa2_fwd_kvcache_mla_varlen_q8).  VQ is a template parameter, instantiated in fa2_decode_mla8_v.hip
// (FA2_DECODE_VARLEN_Q) alone; the argument struct of the fixed unit is what it was.  Q and O are packed (total_q, H, d) / (total_q, H,
// d_v), L is (H, total_q), sequence b owns n_q(b) rows from start(b) on (fa2_varlen_seq).  The query tiling is fa2_decode_mla16.hip's:
//   Rows.    The g n_q(b) rows of one (sequence, KV head) are flattened POSITION-major, row = position * g + head-in-group, 64 to a
//            workgroup: tile t covers the contiguous positions [q0, q1) = [64 t / g, min((64 t + 63) / g + 1, n_q(b))) -- g = 128 two
//            tiles a token, g = 16 four positions a tile, g = 72 a tile that straddles positions unevenly.  Rows past the sequence's last
//            repeat that row and are dropped: no neighbour's packed row is read or written.
//   Grid.    (num_splits * ceil(g max_seqlen_q / 64), H_kv, B).  Sequence b takes its (split, tile) pairs rotated by b along x (a
//            bijection of the grid), so that the tiles that have rows do not sit gridDim.x workgroup ids apart where short sequences
//            stand beside a long one (fa2_decode_mla16.hip has the measurement).  A tile with 64 t >= g n_q(b) leaves at once, before
//            any barrier, and writes nothing.
//   Band.    That of n_q(b) and N_k(b) (fa2_varlen_band), a row's lo / hi from its own position in the sequence.  The split's key
//            range is clipped to the band of the tile's own [q0, q1) -- kb0 stays on a 64-key boundary, so the keys are tiled as the
//            fixed call tiles them -- and the band-edge test of a key tile (lo_max, hi_min) comes from q1 - 1 and q0.  Whole key tiles
//            outside the band are neither loaded nor looked up in the block table.
//   Output.  One split: O to packed row start + position, L to head * l_head_stride + start + position.  Otherwise the partial row is
//            split * total_q * H + (start + position) * H + head, what the combine reads under cu_q.
// start, n_q(b), q0, q1 and the descales are uniform over the workgroup: scalar loads, scalar registers.  A row's arithmetic does not
// depend on its tile-mates and a skipped key tile is one whose every score is masked (P8 = 0, factor 1), so the rows of sequence b are
// the fixed call's on that sequence alone, bit for bit at the same num_splits.  With VQ false q0 = 0, q1 = N_q, start = 0, rows are
// head-major as above and every expression below is the fixed kernel's.
#include "fa2_decode.h"
#include "fa2_mfma.h"

#ifndef FA2_DECODE_VARLEN_Q
#define FA2_DECODE_VARLEN_Q 0
#endif
namespace {

struct DecodeMla8Args {
    const char *Q, *K;
    char *O;
    float *L;
    int64_t qs[3], ks[3], os[3];  // B, H, N strides in BYTES (d stride is 1 element); V is K
    int64_t ls[2];                // L strides in elements
    const int32_t *seqlens;
    int H, g, N_q, S_k, causal, wl, wr, num_splits, row_tiles;
    float *o_part, *l_part;
    float c_log2e;  // scale * log2(e) > 0
    const int32_t *table;  // paged cache only: entry [b, i] at b * table_stride + i; ks[0] is the block stride
    int64_t table_stride;
    int page_size, num_blocks;
    const float *qd, *kd, *vd;  // descales at [b * s[0] + h_kv * s[1]], null = 1
    int64_t qds[2], kds[2], vds[2];
#if FA2_DECODE_VARLEN_Q
    // VQ only (the struct of the fixed unit is what it was): B + 1 offsets into the packed rows; qs[0] = os[0] = ls[0] = 0, N_q holds
    // max_seqlen_q
    const int32_t *cu_q;
    int total_q;
#endif
};

constexpr int kD = 576, kDV = 512, kBC = 64;
constexpr int kCPR = kD / 16;        // 36 16-byte chunks per cache row
constexpr int kKS = kD / 64;         // 9 k-steps of the score
constexpr int kRowB = 640;           // LDS row: 576 B + 64 B of padding
constexpr int kTileB = kBC * kRowB;  // 40 KiB
constexpr int kPOff = 2 * kTileB;    // P8 of the tile: [key block][half][row] x 16 B
constexpr int kXmOff = kPOff + 4096; // [2][64] floats: a row's maximum over each key block
constexpr int kCfOff = kXmOff + 512; // [64]: the rescale factor of the step
constexpr int kXlOff = kCfOff + 256; // [2][64]: a row's sum over each key block's keys (epilogue)
constexpr int kMfOff = kXlOff + 512; // [64]: a row's maximum (epilogue)
constexpr int kSmem = kMfOff + 256;
constexpr int kStage = kCPR * kBC / 256;  // 9 16-byte loads per thread and tile
static_assert(kStage == 9 && kSmem <= 160 * 1024, "two tile buffers in one CU's LDS");

__device__ __forceinline__ int swz8(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2) | ((row >> 2) & 1); }
// Byte offset of 16-byte chunk `ch` (< 36) of row `row` in a tile buffer.
__device__ __forceinline__ int lds_off(int row, int ch) { return row * kRowB + ((ch ^ swz8(row)) << 4); }

// T: O's dtype.  VQ: packed queries, query-tiled, rows position-major (the file's head).
template <typename T, bool PAGED, bool VQ> __global__ __launch_bounds__(256, 1) void fa2_decode_mla8_kernel(const DecodeMla8Args a) {
    using M = F8<true>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = wave & 1, rb = wave >> 1;  // S phase: key block, row block
    const int i = lane & 31, h = lane >> 5;
    const int hk = blockIdx.y, b = blockIdx.z;
    unsigned bx = blockIdx.x;
    if constexpr (VQ) {  // sequence b's (split, tile) pairs rotated by b along x: a bijection of the grid (the file's head)
        bx += blockIdx.z % gridDim.x;  // (gridDim.x <= 128 splits * 2^18 row tiles: the sum stays far inside 32 bits)
        bx -= bx >= gridDim.x ? gridDim.x : 0;
    }
    const int split = bx / a.row_tiles, rt = bx - split * a.row_tiles;
    // N_q: the query count of the mask and of the rows, from packed row `start` on; [q0, q1): the positions the tile's rows lie in
    int N_q = a.N_q, start = 0;
    if constexpr (VQ) {
#if FA2_DECODE_VARLEN_Q
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.N_q, start, N_q);
#endif
        if (rt * 64 >= a.g * N_q) return;  // no rows: nothing to write, no partials (uniform: before any barrier)
    }
    const int R = a.g * N_q;
    const int q0 = VQ ? rt * 64 / a.g : 0;
    const int q1 = VQ ? ((rt * 64 + 63) / a.g + 1 < N_q ? (rt * 64 + 63) / a.g + 1 : N_q) : N_q;

    int NK, k0, k1, wl, wr;
    fa2_decode_split(a.seqlens, b, a.S_k, a.num_splits, split, NK, k0, k1);
    fa2_varlen_band(N_q, NK, a.causal, a.wl, a.wr, wl, wr);
    // the keys of the split that the band of any query position of the tile touches: [kb0, ke), kb0 on a 64-key boundary
    const int lo_t = q0 - wl;
    const int kb0 = lo_t > k0 ? (lo_t & ~63) : k0;  // (k0 is a multiple of 64)
    const int ke = q1 + wr < k1 ? q1 + wr : k1;
    const int nt = ke > kb0 ? (ke - kb0 + kBC - 1) / kBC : 0;

    // ---- S phase: this lane's row (head of the group, query position); padding rows repeat the last row and are not stored.
    // Fixed N_q: row = head * N_q + position.  VQ: row = position * g + head.
    const int srow = rt * 64 + rb * 32 + i;
    const int srowc = srow < R ? srow : R - 1;
    const int sdiv = srowc / (VQ ? a.g : N_q);
    const int srem = srowc - sdiv * (VQ ? a.g : N_q);
    const int shg = VQ ? srem : sdiv, sqi = VQ ? sdiv : srem;

    // ---- Q fragments: B operand of S^T = K Q^T.  Lane (i, h), k-step s: Q[row][16 (4s + h) ..+15] | Q[row][16 (4s + 2 + h) ..+15]
    i32x8 qf[kKS];
    {
        const char *qp = a.Q + b * a.qs[0] + (int64_t)(hk * a.g + shg) * a.qs[1] + (int64_t)(start + sqi) * a.qs[2] + h * 16;
#pragma unroll
        for (int s = 0; s < kKS; ++s) {
            const u32x4 qa = *(const u32x4 *)(qp + s * 64), qb = *(const u32x4 *)(qp + s * 64 + 32);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                qf[s][e] = (int)qa[e];
                qf[s][4 + e] = (int)qb[e];
            }
        }
    }

    // ---- staging map.  Wave w stages tile rows 16w .. 16w + 15: pass ps < 9 is chunk f % 36 of row 16w + f / 36, f = 64 ps + lane
    const char *kg_w = a.K + hk * a.ks[1] + (PAGED ? 0 : b * a.ks[0] + (int64_t)kb0 * a.ks[2]) + (int64_t)(16 * wave) * a.ks[2];
    auto f_row = [&](int ps) { return (64 * ps + lane) / kCPR; };  // < 16
    auto f_ch = [&](int ps) { return (64 * ps + lane) % kCPR; };
    // paged: the walk over the pages as in fa2_decode_mla16.hip: the tiles are taken in order, 64 keys on a multiple of 64
    int pg_i = 0, pg_row = 0;
    const int32_t *tab = nullptr;
    if constexpr (PAGED) {
        pg_i = kb0 / a.page_size;
        pg_row = kb0 - pg_i * a.page_size;
        tab = a.table + b * a.table_stride;
    }
    u32x4 sreg[kStage];
    auto stage_load = [&](int t) {
        const int rel = t * kBC;  // the tile's first key, relative to kb0
        int64_t toff = (int64_t)rel * a.ks[2];
        if constexpr (PAGED) {
            toff = 0;
            // one scalar load per tile; the entry of a tile at or past the split's end is not part of the problem: not loaded
            if (kb0 + rel < ke) toff = (int64_t)fa2_decode_page(tab, pg_i, a.num_blocks) * a.ks[0] + (int64_t)pg_row * a.ks[2];
            pg_row += kBC;
            if (pg_row >= a.page_size) {
                pg_row = 0;
                ++pg_i;
            }
        }
#pragma unroll
        for (int ps = 0; ps < kStage; ++ps) {
            const int row = f_row(ps);
            const bool ok = kb0 + rel + 16 * wave + row < ke;  // past the split's end (<= N_k): zeros, never read
            sreg[ps] = ok ? *(const u32x4 *)(kg_w + toff + (int64_t)row * a.ks[2] + f_ch(ps) * 16) : u32x4{0, 0, 0, 0};
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int ps = 0; ps < kStage; ++ps)
            *(LDS_PTR(u32x4))(lds + buf * kTileB + lds_off(16 * wave + f_row(ps), f_ch(ps))) = sreg[ps];
    };

    // ---- per-lane LDS offsets.  K row read: row 32kb + i, chunks 4s + h and 4s + 2 + h.  V transposed read (ds_read_b64_tr_b8): in
    // its 16-lane group (w = column half of the 32-column block) lane idx addresses key_e (e = idx >> 1) = 8 (e >> 2) + 4 h + (e & 3)
    // of a 16-key step, columns 128 wave + 32 db + 16 w + 8 (idx & 1) .. + 7
    const int k_row = 32 * kb + i, k_swz = swz8(k_row);
    int v_off[4];
    {
        const int w = (lane >> 4) & 1, idx = lane & 15, e = idx >> 1, p8 = idx & 1;
        const int key = 8 * (e >> 2) + 4 * h + (e & 3);  // + 16 q: swz8 unchanged
#pragma unroll
        for (int db = 0; db < 4; ++db) v_off[db] = lds_off(key, 8 * wave + 2 * db + w) + 8 * p8;
    }
    const int p_wr = kPOff + kb * 2048 + h * 1024 + (32 * rb + i) * 16;
    const int p_rd = kPOff + h * 1024 + i * 16;  // + 2048 kb, + 512 rbp
    LDS_PTR(float) xm = (LDS_PTR(float))(lds + kXmOff);
    LDS_PTR(float) cf = (LDS_PTR(float))(lds + kCfOff);
    LDS_PTR(float) xl = (LDS_PTR(float))(lds + kXlOff);
    LDS_PTR(float) mf = (LDS_PTR(float))(lds + kMfOff);

    f32x16 o[4][2];  // [32 value columns 128w + 32db ..][row block]
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int rbp = 0; rbp < 2; ++rbp)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][rbp][r] = 0.0f;
    float m = -INFINITY, lsum = 0.0f;  // of the S-phase row, lsum over this wave's key block only
    // one scalar load per descale and workgroup.  S = (scale qd kd) Q8 K8^T; vd waits in a scalar register for the epilogue
    const float c = a.c_log2e * fa2_decode_descale(a.qd, a.qds[0], a.qds[1], b, hk) * fa2_decode_descale(a.kd, a.kds[0], a.kds[1], b, hk);
    const float vd = fa2_decode_descale(a.vd, a.vds[0], a.vds[1], b, hk);
    // this row's visible keys [lo, hi], and whether a tile can meet a band edge of any row
    const int lo = sqi - wl, hi = (sqi + wr) < (ke - 1) ? (sqi + wr) : (ke - 1);
    const int lo_max = q1 - 1 - wl, hi_min = (q0 + wr) < (ke - 1) ? (q0 + wr) : (ke - 1);

    if (nt > 0) {
        stage_load(0);
        stage_write(0);
    }
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const bool more = t + 1 < nt;
        const int cur = (t & 1) * kTileB;
        if (more) stage_load(t + 1);  // in flight under the S phase and the softmax
        const int tk0 = kb0 + t * kBC;

        // ---- S^T = K . Q^T: this wave's 32 keys x 32 rows
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) {
            const u32x4 ka = *(LDS_PTR(u32x4))(lds + cur + k_row * kRowB + (((4 * ks + h) ^ k_swz) << 4));
            const u32x4 kc = *(LDS_PTR(u32x4))(lds + cur + k_row * kRowB + (((4 * ks + 2 + h) ^ k_swz) << 4));
            i32x8 kf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kf[e] = (int)ka[e];
                kf[4 + e] = (int)kc[e];
            }
            s = M::mfma64(kf, qf[ks], s);
        }
        // ---- band and tail mask, selected: key(r) = tk0 + 32kb + 4h + (r & 3) + 8 (r >> 2)
        if (tk0 < lo_max || tk0 + kBC - 1 > hi_min) {
            const int kl = lo - (tk0 + 32 * kb + 4 * h), kh = hi - (tk0 + 32 * kb + 4 * h);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = (r & 3) + 8 * (r >> 2);
                if (key < kl || key > kh) s[r] = -INFINITY;
            }
        }
        // ---- the row's maximum over the 64 keys: this key block's, then the other wave's through LDS
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (h == 0) xm[kb * 64 + 32 * rb + i] = mx;
        __syncthreads();  // (every P.V read of the last step's tile, P and factors has retired as well)
        mx = fmaxf(mx, xm[(kb ^ 1) * 64 + 32 * rb + i]);
        // ---- online softmax.  While a row's maximum is -inf (no visible key so far) P and the rescale factor are 0.
        const float m_new = fmaxf(m, mx * c);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;
        const float coeff = __builtin_amdgcn_exp2f(m - m_use);
        m = m_new;
        float rs = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -m_use));
            rs += p;            // the unrounded p
            s[r] = p * 256.0f;  // exact
        }
        lsum = lsum * coeff + rs;
        // registers 0..15 in order are k slots 16kb .. 16kb + 15 of the B fragment of lane (i, h), row block rb
        {
            u32x4 pw;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int w = M::template cvt_pk<false>(s[4 * q + 0], s[4 * q + 1], 0);
                w = M::template cvt_pk<true>(s[4 * q + 2], s[4 * q + 3], w);
                pw[q] = (unsigned)w;
            }
            *(LDS_PTR(u32x4))(lds + p_wr) = pw;
        }
        if (kb == 0 && h == 0) cf[32 * rb + i] = coeff;
        if (more) stage_write((t + 1) & 1);  // the other buffer: its last readers (P.V of step t - 1) are behind the barrier above
        __syncthreads();

        // ---- O^T += V^T . P^T over this wave's 128 value columns, both row blocks
        {
            const float c0 = cf[i], c1 = cf[32 + i];
            if (__any(c0 != 1.0f || c1 != 1.0f)) {
#pragma unroll
                for (int db = 0; db < 4; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        o[db][0][r] *= c0;
                        o[db][1][r] *= c1;
                    }
            }
        }
        i32x8 pf[2];
#pragma unroll
        for (int rbp = 0; rbp < 2; ++rbp) {
            const u32x4 pa = *(LDS_PTR(u32x4))(lds + p_rd + 512 * rbp), pb = *(LDS_PTR(u32x4))(lds + p_rd + 512 * rbp + 2048);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pf[rbp][e] = (int)pa[e];
                pf[rbp][4 + e] = (int)pb[e];
            }
        }
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            i32x8 va;
#pragma unroll
            for (int q = 0; q < 4; ++q) {  // keys 16q + ...: k slots 8q .. 8q + 7
                const i32x2 vf = __builtin_amdgcn_ds_read_tr8_b64_v2i32((LDS_PTR(i32x2))(lds + cur + q * 16 * kRowB + v_off[db]));
                va[2 * q] = vf[0];
                va[2 * q + 1] = vf[1];
            }
            o[db][0] = M::mfma64(va, pf[0], o[db][0]);
            o[db][1] = M::mfma64(va, pf[1], o[db][1]);
        }
    }

    // ---- the rows' sums and maxima to the P.V lanes (a region of their own: no barrier before the writes)
    {
        const float lw = lsum + __shfl_xor(lsum, 32, 64);
        if (h == 0) {
            xl[kb * 64 + 32 * rb + i] = lw;
            if (kb == 0) mf[32 * rb + i] = m;
        }
    }
    __syncthreads();

    // ---- epilogue.  Lane (i, h) owns rows 32rbp + i of the tile, columns 128w + 32db + 8g + 4h .. +3 for g = 0..3.
#pragma unroll
    for (int rbp = 0; rbp < 2; ++rbp) {
        const int row = rt * 64 + 32 * rbp + i;
        if (row >= R) continue;
        const int ediv = row / (VQ ? a.g : N_q);  // (recomputed, not carried from the S phase: no register lives across the loop)
        const int erem = row - ediv * (VQ ? a.g : N_q);
        const int hg = VQ ? erem : ediv, qi = VQ ? ediv : erem;
        const int head = hk * a.g + hg;
        const float l = xl[32 * rbp + i] + xl[64 + 32 * rbp + i];
        const float mr = mf[32 * rbp + i];
        const bool seen = l > 0.0f;
        const float inv = seen ? vd * 0.00390625f / l : 0.0f;  // O = vd 2^-8 (P8 V8) / l, in fp32
        if (a.num_splits == 1) {
            char *op = a.O + b * a.os[0] + head * a.os[1] + (int64_t)(start + qi) * a.os[2] + (128 * wave + 4 * h) * 2;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    typedef __attribute__((ext_vector_type(4))) T Tx4;
                    Tx4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (T)(o[db][rbp][4 * g + j] * inv);
                    *(u32x2 *)(op + db * 64 + g * 16) = __builtin_bit_cast(u32x2, v);
                }
            if (wave == 0 && h == 0) a.L[b * a.ls[0] + head * a.ls[1] + start + qi] = seen ? mr + __builtin_amdgcn_logf(l) : INFINITY;
        } else {
#if FA2_DECODE_VARLEN_Q
            const int64_t rows = (int64_t)a.total_q * a.H;  // the packed partial rows: token * H + head
            const int64_t prow = (int64_t)split * rows + (int64_t)(start + qi) * a.H + head;
#else
            const int64_t rows = (int64_t)gridDim.z * a.H * N_q;
            const int64_t prow = (int64_t)split * rows + ((int64_t)b * a.H + head) * N_q + qi;
#endif
            float *op = a.o_part + prow * kDV + 128 * wave + 4 * h;
            float invp = inv;
            // VQ: the products of this branch are kept apart from the one-split branch's, as in fa2_decode_mla16.hip: a product the
            // compiler hoists above both branches is rounded twice on its way to f16 where the fixed kernel's v_fma_mixlo_f16 rounds
            // once, against the bit-for-bit equality with the fixed call
            if constexpr (VQ) asm volatile("" : "+v"(invp));
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = o[db][rbp][4 * g + j] * invp;
                    *(f32x4 *)(op + db * 32 + g * 8) = v;
                }
            if (wave == 0 && h == 0) a.l_part[prow] = seen ? mr + __builtin_amdgcn_logf(l) : -INFINITY;
        }
    }
}

constexpr bool kVQ = FA2_DECODE_VARLEN_Q != 0;

template <typename T, bool PAGED> int launch_t(const Fa2DecodeProblem &p, const DecodeMla8Args &a) {
    const long long gx = (long long)p.num_splits * a.row_tiles;
    if (gx > 0x7fffffffLL) {
        fa2_set_error("kvcache mla8 kernel: grid too large (num_splits * row tiles = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    static Fa2DeviceLatch attr_done;  // more than 64 KiB of dynamic LDS: opt in, once per device
    if (attr_done.need()) {
        (void)hipFuncSetAttribute((const void *)fa2_decode_mla8_kernel<T, PAGED, kVQ>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem);
        attr_done.mark();
    }
    const dim3 grid((unsigned)gx, p.H_kv, p.B), block(256);
    hipLaunchKernelGGL((fa2_decode_mla8_kernel<T, PAGED, kVQ>), grid, block, kSmem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache mla8 kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <typename T> int launch_p(const Fa2DecodeProblem &p, const DecodeMla8Args &a) {
    return p.table ? launch_t<T, true>(p, a) : launch_t<T, false>(p, a);
}

bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

// (packed queries: N_q holds max_seqlen_q, so the row bound below is the grid's, and qs / os are the packed rows' strides)
bool supports(const Fa2DecodeProblem &p) {
    if (!fa2_decode_mla8_shape(p.d, p.d_v, p.q_dtype, p.kv_dtype) || (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16)) return false;
    if (p.kv_format != 0 || (p.cu_q != nullptr) != kVQ || p.indices) return false;
    if (p.V != p.K) return false;  // the value operand is read from K's LDS image
    for (int k = 0; k < 4; ++k)
        if (p.vs[k] != p.ks[k]) return false;
    if (!(p.scale > 0.0f) || !(p.scale < INFINITY)) return false;
    if ((int64_t)(p.H / p.H_kv) * p.N_q > (1 << 24)) return false;  // (rows of a KV group are counted in 32 bits)
    if (p.qs[3] != 1 || p.ks[3] != 1 || p.os[3] != 1) return false;
    // 16-byte vector loads of Q and K rows (bytes), 8-byte stores of O: every row start must stay aligned
    for (int k = 0; k < 3; ++k)
        if ((p.qs[k] & 15) || (p.ks[k] & 15) || (p.os[k] & 7)) return false;
    if (!aligned16(p.Q) || !aligned16(p.K) || !aligned16(p.O)) return false;
    if (p.num_splits > 1 && !aligned16(p.o_part)) return false;
    if (p.table && p.page_size % FA2_KVCACHE_KEY_TILE != 0) return false;  // a 64-key tile must lie inside one page
    return true;
}

int launch(const Fa2DecodeProblem &p) {
    if (!supports(p)) {
        fa2_set_error("kvcache mla8 kernel: needs e4m3fn Q over an e4m3fn cache (the generic kernel takes e5m2), d = 576 and d_v = 512, f16/bf16 "
                      "O, V aliasing K (the same pointer and strides), unit d-stride, 16-byte aligned rows of Q and K (base and strides "
                      "multiples of 16 bytes), 16-byte aligned O rows (and workspace), scale > 0%s",
                      p.table ? ", page_size % 64 == 0 for a paged cache (other page sizes: the generic kernel)" : "");
        return FA2_ERR_UNSUPPORTED;
    }
    DecodeMla8Args a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K;
    a.O = (char *)p.O; a.L = (float *)p.L;
    for (int k = 0; k < 3; ++k) { a.qs[k] = p.qs[k]; a.ks[k] = p.ks[k]; a.os[k] = p.os[k] * 2; }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.seqlens = p.seqlens;
    a.H = p.H; a.g = p.H / p.H_kv; a.N_q = p.N_q; a.S_k = p.S_k; a.causal = p.causal; a.wl = p.wl; a.wr = p.wr;
    a.num_splits = p.num_splits;
    a.row_tiles = (int)(((int64_t)a.g * p.N_q + 63) / 64);
    a.o_part = p.o_part; a.l_part = p.l_part;
    a.c_log2e = (float)((double)p.scale * FA2_LOG2E);
    a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.qd = p.qd; a.kd = p.kd; a.vd = p.vd;
    for (int k = 0; k < 2; ++k) { a.qds[k] = p.qds[k]; a.kds[k] = p.kds[k]; a.vds[k] = p.vds[k]; }
#if FA2_DECODE_VARLEN_Q
    a.cu_q = p.cu_q; a.total_q = p.total_q;
#endif
    return p.dtype == FA2_DTYPE_BF16 ? launch_p<__bf16>(p, a) : launch_p<_Float16>(p, a);
}

}  // namespace

#if FA2_DECODE_VARLEN_Q
bool fa2_decode_mla8_v_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mla8_v(const Fa2DecodeProblem &p) { return launch(p); }
#else
bool fa2_decode_mla8_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mla8(const Fa2DecodeProblem &p) { return launch(p); }
#endif
