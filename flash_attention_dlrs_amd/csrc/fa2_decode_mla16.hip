// fa2_decode_mla16.hip -- KV-cache decode over a shared latent cache (fa2_fwd_kvcache_mla and _mla_fp8, FA2_KVCACHE_VARIANT_MLA16):
// multi-head latent attention in its absorbed form, f16 / bf16 (the cache alike, or fp8 storage), d = 576 (512 latent + 64 rotary
// columns), d_v = 512, V = K[..., :512].
//
// One workgroup of four waves handles one (split, 64-row tile of a KV group, KV head, sequence): the grid is
// (num_splits * row_tiles, H_kv, B), row r = head-in-group * N_q + query as in fa2_decode_mfma16.hip, a last tile with fewer
// than 64 rows computing its padding rows (the last row again) and dropping them.  A second row tile reads the same keys again.
//
// Per step the workgroup takes ONE 64-key tile of the latent cache, staged once: 64 rows of 1,152 B in an LDS image of 1,280-B
// rows (a multiple of 256 B, so the 16-bit tile swizzle (fa2_mfma.h) at d = 128 -- a function of row & 15 on the low four bits
// of the 16-byte chunk index -- keeps the K row reads and the transposed V reads conflict-free; the 128 B of padding per row are
// never read).  The score reads all 72 chunks of a row, the value side columns 0..511 of the SAME image through
// ds_read_b64_tr_b16: the value operand is never fetched a second time.
//
//   S phase.   Wave w owns key block w & 1 and row block w >> 1 of S^T = K Q^T on v_mfma_f32_32x32x16: 36 k-steps, its Q
//              fragments (36 x 4 registers) resident.
//   Softmax.   The two key blocks of a row exchange their maxima through LDS; then the online softmax of the other decode kernels
//              (exp2 domain, masked scores SELECTED to -inf, P rounded to the I/O dtype).  P of the 64 x 64 tile goes to LDS in
//              the B-fragment order of the P.V MFMAs (rows of 144 B: conflict-free 16-byte reads), beside the per-row rescale
//              factors.
//   P.V phase. Wave w owns value columns [128 w, 128 w + 128) for all 64 rows: 4 x 2 accumulator tiles (128 registers), 32 MFMAs
//              per step, each V fragment used for both row blocks.
//
// Staging goes through registers while the previous tile is computed (single-buffered, 18 x 16 bytes per thread): a wave loads
// 16 rows, chunks 0..63 of a row with one instruction (1 KiB contiguous) and the last 8 chunks of 8 rows with another, so no
// load crosses a row.  Addresses are 64-bit per thread.
//
// fp8 latent cache (fa2_fwd_kvcache_mla_fp8).  The cache element type C is a template parameter: T itself, or OCP e4m3fn / e5m2 with
// per-(b, h_kv) descales kd, vd.  Only staging differs: a row is 576 B = 36 loads of 16 bytes, a load holds 16 elements that
// CacheCvt (fa2_decode.h) converts exactly to the two 16-byte LDS chunks 2c and 2c + 1 of the same image, so a thread stages 9
// loads per tile instead of 18.  A wave's 16 rows are 576 loads = 9 passes of 64 lanes under the flat index f = 64 pass + lane ->
// (row f / 36, load f % 36): consecutive lanes read consecutive 16-byte pieces (a pass is 1 KiB in at most three rows) and no load
// crosses a row.  Of its two chunks a lane writes chunk 2c + (c >> 2 & 1) first and the other one second: the eight lanes of a
// ds_write_b128 group then hit eight distinct 16-byte slots of the 128-B bank row (2c alone would be four slots, twice each), as
// the 16-bit map's 64 consecutive chunks do; only a group that straddles a row keeps a 2-way conflict.  The descales are folded,
// not applied per element: kd into the softmax scale of the workgroup, vd into the fp32 normalisation of the output, before it
// is rounded or written as a partial (K and V are the same bytes, the two descales still independent scalars).  A row past the
// split's end is zeros before the conversion: no stale byte, NaN and inf patterns included, is ever converted.
//
// Stale cache contents: a key at or past the split's end (<= N_k(b)) is not loaded -- its row is written to LDS as zeros and its
// score is selected to -inf -- so what lies behind cache_seqlens[b] is never read.  Paged cache: page_size % 64 == 0, a key
// tile lies inside one page, its table entry is one scalar load, clamped to [0, num_blocks - 1]; the entry of a tile at or past
// the split's end is not loaded.
//
// Output: num_splits == 1 writes O / l and L = m + log2 l in the I/O dtype (a row without a visible key: O = 0, L = +inf);
// otherwise every (split, row) writes the normalised fp32 partial (an empty split: 0 and -inf) for fa2_decode_combine.hip.
// Vector stores only, no atomics, no hand-off between workgroups.
//
// Variable-length queries (fa2_fwd_kvcache_mla_varlen).  VQ is a template parameter, instantiated in fa2_decode_mla16_v.hip
// (FA2_DECODE_VARLEN_Q) alone: Q and O are packed (total_q, H, d) / (total_q, H, d_v), L is (H, total_q), sequence b owns n_q(b)
// rows from start(b) on (fa2_varlen_seq).  The g n_q(b) rows of one (sequence, KV head) are flattened POSITION-major, row =
// position * g + head-in-group, and a workgroup owns rows [64 t, 64 t + 64) of them: every tile but a sequence's last is full for
// any g, and a tile covers the contiguous positions [q0, q1) = [64 t / g, min((64 t + 63) / g + 1, n_q(b))).  The grid's x axis is
// (split, ceil(g max_seqlen_q / 64) tiles); a tile with 64 t >= g n_q(b) leaves at once, before any barrier, and writes nothing.
// (Sequence b takes its (split, tile) pairs rotated by b along x, so that the tiles with rows of short sequences do not sit a fixed
// gridDim.x workgroup ids apart: see the kernel's head.)
// Padding rows repeat the sequence's last row and are dropped: no neighbour's packed row is read or written.  The mask is the band
// of n_q(b) and N_k(b), the row's position counted in the SEQUENCE; the split's key range is clipped to the band of the tile's own
// [q0, q1), whole 64-key tiles outside it neither loaded nor looked up.  The partial row is split * total_q * H + (start +
// position) * H + head, what the combine expects for cu_q.  With VQ false q0 = 0, q1 = N_q, start = 0, rows are head-major as
// above and every expression below is the fixed-N_q kernel's.
//
// Per-query key lists (fa2_fwd_kvcache_mla_sparse).  SP is a template parameter, instantiated in fa2_decode_mla16_s.hip
// (FA2_DECODE_SPARSE) alone; the argument struct of the other units is what it was.  Every (sequence, KV head, query position)
// attends over the keys its list of topk int32 entries names.  A workgroup owns 64 HEADS of one (sequence, KV head, position) --
// ceil(g / 64) head tiles, padding rows repeat the group's last head and are dropped -- so its 64 rows share ONE list; the grid is
// (B * N_q * num_splits * head tiles, H_kv), the workgroups of one list on consecutive ids, and holds B * N_q in the hundreds of
// thousands (a sparse prefill chunk is B = 1, N_q in the thousands).  With N_q = 1 and `start` the position, every row expression of
// the fixed-N_q kernel holds as it stands.  The splits run over the SLOTS of the list (fa2_decode_split_slots): [k0, k1), kb0, ke and
// a tile's tk0 are slot numbers there, and a step takes the 64 slots of a tile.
//   The list.   A wave reads the 64 entries of a tile once, one slot per lane (256 B coalesced with unit slot stride).  An entry j is
//               a key where 0 <= j < N_k(b) and its slot lies before the split's end; the validity of the 64 slots is a 64-bit wave
//               mask.  Two tiles ahead of the one in LDS: the entries of tile t + 3 are issued while the rows of tile t + 1 are
//               loaded, those of tile t + 2 are judged then and (paged) their table entries issued -- entry j is row j % page_size of
//               page table[b][j / page_size], one lookup per lane, ANY page size, clamped into the pool where it is used -- so neither
//               dependent load is waited for in the step that issues it.
//   Staging.    Each lane forms the 64-bit offset of its slot's row, position * row stride (+ page * block stride).  A wave brings
//               its 16 rows' offsets to lanes 0..15 with one shuffle; row `it` then takes its offset with a lane read at a constant
//               lane and is loaded as the dense kernel loads it (1 KiB + the 128-B tail, whose rows take theirs with a shuffle, as
//               do the passes of the fp8 map, which cross rows).  The mask gates the loads: a slot that is no key is never turned
//               into a table index or an address, its row is zeros in LDS.
//   S phase.    The mask replaces the band test, a bit per key(r): a slot that is no key is selected to -inf.  A key listed twice is
//               staged and counted twice.  A row without a valid entry: O = 0, L = +inf.
// The LDS image, the swizzle, the S / softmax / P.V phases, the epilogue and the partial layout are the dense kernel's: on the
// identity list over N_k = topk keys O and L equal the dense call's bit for bit at the same num_splits.
//
// Per-query key lists of packed queries (fa2_fwd_kvcache_mla_sparse_varlen).  SP and VQ together, instantiated in
// fa2_decode_mla16_sv.hip alone: Q, O, L and the partial rows are the packed call's, the list of packed row t is entry [t, h_kv] and
// names key positions of the sequence that owns t.  The x axis is (t * num_splits + split) * head tiles + head tile over total_q
// tokens, however they fall into sequences.  The workgroup finds the owner of its row (fa2_varlen_owner: a uniform binary search
// over cu_q on scalar loads, at most 16 steps, then fa2_varlen_seq) and takes N_k(b), the table row and the descales of that b; a row
// no sequence owns leaves at once, before any barrier, and writes nothing -- what the query-tiled packed form does with a tile
// without rows.  With `start` the packed row and N_q = 1 every expression below is the list-addressed kernel's: the query tiling of
// VQ (the rotation along x, position-major rows, [q0, q1)) is taken with VQ && !SP alone, the packed partial layout with VQ.
#include "fa2_decode.h"
#include "fa2_mfma.h"

#ifndef FA2_DECODE_VARLEN_Q
#define FA2_DECODE_VARLEN_Q 0
#endif
#ifndef FA2_DECODE_SPARSE
#define FA2_DECODE_SPARSE 0
#endif

namespace {

struct DecodeMlaArgs {
    const char *Q, *K;
    char *O, *L;
    int64_t qs[3], ks[3], os[3];  // B, H, N strides in BYTES (d stride is 1 element); V is K
    int64_t ls[2];                // L strides in elements
    const int32_t *seqlens;
    int H, g, N_q, S_k, causal, wl, wr, num_splits, row_tiles;
    float *o_part, *l_part;
    float c_log2e;  // scale * log2(e) > 0
    const int32_t *table;  // paged cache only: entry [b, i] at b * table_stride + i; ks[0] is the block stride
    int64_t table_stride;
    int page_size, num_blocks;
    const float *kd, *vd;  // fp8 cache only: descales at [b * kds[0] + h_kv * kds[1]], null = 1
    int64_t kds[2], vds[2];
    const int32_t *cu_q;  // VQ only: B + 1 offsets into the packed rows; qs[0] = os[0] = ls[0] = 0, N_q holds max_q
    int total_q;
#if FA2_DECODE_SPARSE
    const int32_t *idx;  // SP only (the struct of the other units is what it was): entry [b, hk, qi, slot] at the element strides is[4]
    int64_t is[4];
    int topk, B;
#endif
};

constexpr int kD = 576, kDV = 512, kBC = 64;
constexpr int kCPR = kD * 2 / 16;    // 72 16-byte chunks per cache row
constexpr int kKS = kD / 16;         // 36 k-steps of the score
constexpr int kRowB = 1280;          // LDS row: 1,152 B + 128 B of padding
constexpr int kTileB = kBC * kRowB;  // 80 KiB
constexpr int kPRowB = 144;          // a row of P: 64 keys x 2 B + 16 B of padding
constexpr int kPOff = kTileB;
constexpr int kXmOff = kPOff + 64 * kPRowB;  // [2][64] floats: a row's maximum over each key block
constexpr int kCfOff = kXmOff + 512;         // [64]: the rescale factor of the step
constexpr int kXlOff = kCfOff + 256;         // [2][64]: a row's sum over each key block's keys (epilogue)
constexpr int kMfOff = kXlOff + 512;         // [64]: a row's maximum (epilogue)
constexpr int kSmem = kMfOff + 256;
constexpr int kStage = kCPR * kBC / 256;     // 18 16-byte loads per thread and tile
constexpr int kLPR8 = kD / 16;               // fp8 cache: 36 16-byte loads per cache row, each two LDS chunks
constexpr int kStage8 = kLPR8 * kBC / 256;   //            9 loads per thread and tile
static_assert(kStage == 18 && kStage8 == 9 && kSmem <= 160 * 1024, "one workgroup per CU");

// Byte offset of 16-byte chunk `ch` (< 72) of row `row` in the tile: the d = 128 swizzle on rows of kRowB bytes.
__device__ __forceinline__ int lds_off(int row, int ch) { return row * kRowB + ((ch ^ swz<128>(row)) << 4); }

template <bool V> struct Bool { static constexpr bool value = V; };  // a compile-time flag as a lambda's argument

// T: Q, O, L and the matrix arithmetic; C: the cache (T, or an fp8 format converted while it is staged).  VQ: packed queries,
// rows position-major.  SP: per-query key lists (the file's head), the rows of a workgroup heads of ONE query position.
template <typename T, typename C, bool PAGED, bool VQ, bool SP>
__global__ __launch_bounds__(256, 1) void fa2_decode_mla16_kernel(const DecodeMlaArgs a) {
    using M = Mma<T>;
    constexpr bool F8 = !__is_same(C, T);
    using frag = typename M::frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kb = wave & 1, rb = wave >> 1;  // S phase: key block, row block
    const int i = lane & 31, h = lane >> 5;
    int bx = blockIdx.x;
    int sp_b = 0, sp_qi = 0;
    if constexpr (SP) {
        // x = ((b * N_q + position) * num_splits + split) * row_tiles + head tile: the workgroups that share a list sit on
        // consecutive ids, and the axis holds B * N_q in the hundreds of thousands (a sparse prefill chunk)
        const int per = a.num_splits * a.row_tiles, tok = bx / per;
        bx -= tok * per;
        if constexpr (VQ) {
#if FA2_DECODE_SPARSE && FA2_DECODE_VARLEN_Q
            // packed: tok < total_q is a packed row.  Its owner, or nothing to do (uniform: before any barrier)
            int st, n;
            if (!fa2_varlen_owner(a.cu_q, a.B, a.total_q, a.N_q, tok, sp_b, st, n)) return;
            sp_qi = tok;  // (qs[0] = os[0] = ls[0] = is[0] = 0: the packed row is the position of every address below)
#endif
        } else {
            sp_b = tok / a.N_q;
            sp_qi = tok - sp_b * a.N_q;
        }
    }
    constexpr bool VT = VQ && !SP;  // the query-tiled packed form
    const int hk = blockIdx.y, b = SP ? sp_b : blockIdx.z;
    if constexpr (VT) {
        // The hardware deals consecutive workgroup ids round the chip's shader engines.  With tile t of every sequence at x = t the
        // tiles that have rows sit gridDim.x ids apart where the sequences are short (one-token decodes beside a long chunk), and
        // where that stride is a multiple of the number of engines they all land on ONE engine's 8 CUs, at one workgroup per CU
        // (measured: 63 one-token sequences under max_seqlen_q = 256 took 955 us, 123 us alone).  So sequence b takes its (split,
        // tile) pairs rotated by b: a long sequence's tiles stay on consecutive ids, the first tiles of consecutive sequences sit
        // gridDim.x - 1 ids apart.  A bijection of the same grid.
        bx += blockIdx.z % gridDim.x;  // (gridDim.x <= 128 splits * 2^18 row tiles: the sum stays far inside an int)
        bx -= bx >= (int)gridDim.x ? (int)gridDim.x : 0;
    }
    const int split = bx / a.row_tiles, rt = bx - split * a.row_tiles;
    // N_q: the query count of the mask and of the rows, from packed row `start` on; [q0, q1): the positions the tile's rows lie in
    int N_q = a.N_q, start = 0;
    if constexpr (SP) {  // one position, `start`, whose g heads are the rows: every row expression below then holds as it stands
        N_q = 1;
        start = sp_qi;
    }
    if constexpr (VT) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.N_q, start, N_q);
        if (rt * 64 >= a.g * N_q) return;  // no rows: nothing to write, no partials (uniform: before any barrier)
    }
    const int R = a.g * N_q;
    const int q0 = VT ? rt * 64 / a.g : 0;
    const int q1 = VT ? ((rt * 64 + 63) / a.g + 1 < N_q ? (rt * 64 + 63) / a.g + 1 : N_q) : N_q;

    int NK, k0, k1;  // SP: [k0, k1) are SLOTS of the list, and so are kb0, ke and tk0 below; there is no band
    int wl = 0, wr = 0, spB = 0;
    [[maybe_unused]] const int32_t *ip = nullptr;  // SP: the list of this (sequence, KV head, position)
    if constexpr (SP) {
#if FA2_DECODE_SPARSE
        fa2_decode_split_slots(a.seqlens, b, a.S_k, a.topk, a.num_splits, split, NK, k0, k1);
        ip = a.idx + b * a.is[0] + hk * a.is[1] + sp_qi * a.is[2];
        spB = a.B;
#endif
    } else {
        fa2_decode_split(a.seqlens, b, a.S_k, a.num_splits, split, NK, k0, k1);
        fa2_varlen_band(N_q, NK, a.causal, a.wl, a.wr, wl, wr);
    }
    // the keys of the split that the band of any query position of the tile touches: [kb0, ke), kb0 on a 64-key boundary
    const int lo_t = q0 - wl;
    const int kb0 = SP ? k0 : lo_t > k0 ? (lo_t & ~63) : k0;  // (k0 is a multiple of 64)
    const int ke = SP ? k1 : q1 + wr < k1 ? q1 + wr : k1;
    const int nt = ke > kb0 ? (ke - kb0 + kBC - 1) / kBC : 0;

    // ---- S phase: this lane's row (head of the group, query position); padding rows repeat the last row and are not stored.
    // Fixed N_q: row = head * N_q + position.  VQ: row = position * g + head.
    const int srow = rt * 64 + rb * 32 + i;
    const int srowc = srow < R ? srow : R - 1;
    const int sdiv = srowc / (VT ? a.g : N_q);
    const int srem = srowc - sdiv * (VT ? a.g : N_q);
    const int shg = VT ? srem : sdiv;
    const int sqi = VT ? sdiv : srem;

    // ---- Q fragments: B operand of S^T = K Q^T.  Lane (i, h) holds Q[row][16ks + 8h .. +7].
    frag qf[kKS];
    {
        const char *qp = a.Q + b * a.qs[0] + (int64_t)(hk * a.g + shg) * a.qs[1] + (int64_t)(start + sqi) * a.qs[2] + h * 16;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) qf[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(qp + ks * 32));
    }

    // ---- staging map.  Wave w stages tile rows 16w .. 16w + 15: pass it < 16 is row 16w + it, chunks 0..63 (one per lane); pass
    // 16 + jb is rows 16w + 8jb + (lane >> 3), chunks 64 + (lane & 7).  (paged: the page's offset joins in stage_load)
    // fp8 cache: pass ps < 9 is load f % 36 of row 16w + f / 36, f = 64 ps + lane (the file's head).
    const int sb_row = 16 * wave + (lane >> 3), sb_ch = 64 + (lane & 7);
    const char *kbase = a.K + hk * a.ks[1] + (PAGED ? 0 : b * a.ks[0] + (SP ? 0 : (int64_t)kb0 * a.ks[2]));
    const char *kg_w = kbase + (int64_t)(16 * wave) * a.ks[2];  // the wave's first row
    const char *kg_a = kg_w + lane * 16;
    const char *kg_b = kbase + (int64_t)sb_row * a.ks[2] + sb_ch * 16;
    auto f8_row = [&](int ps) { return (64 * ps + lane) / kLPR8; };  // < 16
    auto f8_ld = [&](int ps) { return (64 * ps + lane) % kLPR8; };

    // paged: the walk over the pages, as in fa2_decode_mfma16.hip: stage_load takes the tiles in order, a tile is 64 keys on a
    // multiple of 64 and page_size is a multiple of 64, so (pg_i, pg_row) advance by 64 rows per tile and wrap at page_size.
    int pg_i = 0, pg_row = 0;
    const int32_t *tab = nullptr;
    if constexpr (PAGED) {
        if constexpr (!SP) {
            pg_i = kb0 / a.page_size;
            pg_row = kb0 - pg_i * a.page_size;
        }
        tab = a.table + b * a.table_stride;
    }
    // SP: the list walks three tiles ahead of the compute.  `j_b` is the RAW entry of slot (tile, lane) two tiles after the one in
    // LDS, in flight since the last step; sp_advance(tn) takes it for tile tn: its validity becomes the wave mask m_a, its row (in
    // its page) rw_a, the raw table entry e_a is issued, and the entries of tile tn + 1 are issued into j_b.  The next step's
    // stage_load reads rows through (m_a, rw_a, e_a): neither the index load nor the table load is waited for in the step that
    // issues it.  An entry that is no key (outside [0, N_k), or a slot at or past the split's end, which is not even loaded) never
    // becomes a table index or an address: its row is zeros in LDS and its score is selected to -inf through the mask.
    unsigned long long m_cur = 0, m_a = 0;
    int rw_a = 0, e_a = 0, j_b = -1;
    auto sp_idx = [&](int t) {
#if FA2_DECODE_SPARSE
        const int slot = k0 + t * kBC + lane;  // one slot per lane: 256 B of a list with unit slot stride
        if (slot < k1) return ip[slot * a.is[3]];
#endif
        return (int)-1;
    };
    auto sp_advance = [&](int tn) {
        const bool ok = k0 + tn * kBC + lane < k1 && j_b >= 0 && j_b < NK;
        m_a = __ballot(ok);
        rw_a = j_b;
        if constexpr (PAGED) {
            const int pg = j_b / a.page_size;
            rw_a = j_b - pg * a.page_size;
            e_a = ok ? tab[pg] : 0;  // raw: clamped where it is used
        }
        j_b = sp_idx(tn + 1);
    };
    // the byte offset of the row that lane `src` of the wave holds, out of the per-lane offsets `offv` of the tile's 64 rows;
    // U: src is uniform (two lane reads), else two shuffles
    auto sp_off = [&](int64_t offv, int src, auto uniform) {
        constexpr bool U = decltype(uniform)::value;
        const int lo = (int)offv, hi = (int)(offv >> 32);
        const unsigned l = U ? __builtin_amdgcn_readlane(lo, src) : __shfl(lo, src, 64);
        const int u = U ? __builtin_amdgcn_readlane(hi, src) : __shfl(hi, src, 64);
        return (int64_t)u << 32 | l;
    };
    auto sp_offv = [&]() {  // this lane's row of the tile (m_a, rw_a, e_a) describe: position * row stride + (page term), 64-bit
        int64_t offv = (int64_t)rw_a * a.ks[2];
        if constexpr (PAGED) offv += (int64_t)(e_a < 0 ? 0 : (e_a > a.num_blocks - 1 ? a.num_blocks - 1 : e_a)) * a.ks[0];
        return offv;
    };

    u32x4 sreg[F8 ? kStage8 : kStage];
    auto stage_load = [&](int t) {
        if constexpr (SP) {  // tile t is the one (m_a, rw_a, e_a) describe
            const int64_t offv = sp_offv();
            if constexpr (F8) {
#pragma unroll
                for (int ps = 0; ps < kStage8; ++ps) {
                    const int src = 16 * wave + f8_row(ps);
                    const bool ok = (m_a >> src) & 1;
                    const int64_t off = sp_off(offv, src, Bool<false>{});
                    sreg[ps] = ok ? *(const u32x4 *)(kbase + off + f8_ld(ps) * 16) : u32x4{0, 0, 0, 0};
                }
            } else {
                // the wave's own 16 rows brought to lanes 0..15 first (one shuffle): row `it` is then a lane read at a constant
                // lane, its validity a constant bit (16 wave + it as the lane would keep 16 scalar registers alive across the loop)
                const int64_t offw = sp_off(offv, 16 * wave + (lane & 15), Bool<false>{});
                const unsigned mw = (unsigned)(m_a >> (16 * wave));
#pragma unroll
                for (int it = 0; it < 16; ++it) {
                    const bool ok = (mw >> it) & 1;  // uniform
                    const int64_t off = sp_off(offw, it, Bool<true>{});
                    sreg[it] = ok ? *(const u32x4 *)(kbase + off + lane * 16) : u32x4{0, 0, 0, 0};
                }
#pragma unroll
                for (int jb = 0; jb < 2; ++jb) {
                    const bool ok = (m_a >> (sb_row + 8 * jb)) & 1;
                    const int64_t off = sp_off(offv, sb_row + 8 * jb, Bool<false>{});
                    sreg[16 + jb] = ok ? *(const u32x4 *)(kbase + off + sb_ch * 16) : u32x4{0, 0, 0, 0};
                }
            }
            return;
        }
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
        if constexpr (F8) {
#pragma unroll
            for (int ps = 0; ps < kStage8; ++ps) {
                const int row = f8_row(ps);
                const bool ok = kb0 + rel + 16 * wave + row < ke;  // past the split's end (<= N_k): zeros, never read
                sreg[ps] = ok ? *(const u32x4 *)(kg_w + toff + (int64_t)row * a.ks[2] + f8_ld(ps) * 16) : u32x4{0, 0, 0, 0};
            }
        } else {
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const bool ok = kb0 + rel + 16 * wave + it < ke;  // past the split's end (<= N_k): zeros, never read
                sreg[it] = ok ? *(const u32x4 *)(kg_a + toff + (int64_t)it * a.ks[2]) : u32x4{0, 0, 0, 0};
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const bool ok = kb0 + rel + sb_row + 8 * jb < ke;
                sreg[16 + jb] = ok ? *(const u32x4 *)(kg_b + toff + (int64_t)(8 * jb) * a.ks[2]) : u32x4{0, 0, 0, 0};
            }
        }
    };
    auto stage_write = [&]() {
        if constexpr (F8) {  // word j of the load = elements 4j .. 4j + 3 = words 2j, 2j + 1 of the 16-bit row
            using X = CacheCvt<T, C>;
#pragma unroll
            for (int ps = 0; ps < kStage8; ++ps) {
                const u32x4 w = sreg[ps];
                const u32x4 c0 = {X::template cvt<false>(w[0]), X::template cvt<true>(w[0]), X::template cvt<false>(w[1]),
                                  X::template cvt<true>(w[1])};
                const u32x4 c1 = {X::template cvt<false>(w[2]), X::template cvt<true>(w[2]), X::template cvt<false>(w[3]),
                                  X::template cvt<true>(w[3])};
                const int row = 16 * wave + f8_row(ps), ld = f8_ld(ps);
                const bool odd_first = (ld & 4) != 0;  // which of chunks 2 ld, 2 ld + 1 goes first: the bank rule at the file's head
                *(LDS_PTR(u32x4))(lds + lds_off(row, 2 * ld + (odd_first ? 1 : 0))) = odd_first ? c1 : c0;
                *(LDS_PTR(u32x4))(lds + lds_off(row, 2 * ld + (odd_first ? 0 : 1))) = odd_first ? c0 : c1;
            }
        } else {
#pragma unroll
            for (int it = 0; it < 16; ++it) *(LDS_PTR(u32x4))(lds + lds_off(16 * wave + it, lane)) = sreg[it];
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) *(LDS_PTR(u32x4))(lds + lds_off(sb_row + 8 * jb, sb_ch)) = sreg[16 + jb];
        }
    };

    // ---- per-lane LDS offsets.  K row read: row 32kb + i, chunk 2ks + h.  V transposed read (ds_read_b64_tr_b16): lane 4q + p of a
    // 16-lane group supplies row (16ks + 8u + 4h + q), columns 128w + 32db + 16(group & 1) + 4p .. +3.
    const int k_row = 32 * kb + i;
    const int k_swz = ((k_row & 3) << 2) | ((k_row >> 2) & 3);
    int v_off[2][4];
    {
        const int w = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int db = 0; db < 4; ++db)
                v_off[u][db] = lds_off(8 * u + 4 * h + qq, 16 * wave + 4 * db + 2 * w + (pp >> 1)) + 8 * (pp & 1);
    }
    const int p_wr = kPOff + (32 * rb + i) * kPRowB + ((4 * kb + h) << 4);  // + 32 ss: k-step 2kb + ss, half h
    const int p_rd = kPOff + i * kPRowB + (h << 4);                         // + 32 rbp rows, + 32 ks
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
    // fp8: one scalar load per descale and workgroup.  S = (scale kd) Q K8^T; vd waits in a scalar register for the epilogue.
    float c = a.c_log2e, vd = 1.0f;
    if constexpr (F8) {
        c *= fa2_decode_descale(a.kd, a.kds[0], a.kds[1], b, hk);
        vd = fa2_decode_descale(a.vd, a.vds[0], a.vds[1], b, hk);
    }
    // this row's visible keys [lo, hi], and whether a tile can meet a band edge of any row
    const int lo = sqi - wl, hi = (sqi + wr) < (ke - 1) ? (sqi + wr) : (ke - 1);
    const int lo_max = q1 - 1 - wl, hi_min = (q0 + wr) < (ke - 1) ? (q0 + wr) : (ke - 1);

    if (nt > 0) {
        if constexpr (SP) {
            j_b = sp_idx(0);
            sp_advance(0);
            m_cur = m_a;
        }
        stage_load(0);
        if constexpr (SP) sp_advance(1);
        stage_write();
    }
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const bool more = t + 1 < nt;
        if (more) stage_load(t + 1);
        const unsigned long long m_nxt = m_a;  // SP: of tile t + 1
        if constexpr (SP)
            if (more) sp_advance(t + 2);
        const int tk0 = kb0 + t * kBC;

        // ---- S^T = K . Q^T: this wave's 32 keys x 32 rows
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) {
            const u32x4 kf = *(LDS_PTR(u32x4))(lds + k_row * kRowB + (((2 * ks + h) ^ k_swz) << 4));
            s = M::mfma(__builtin_bit_cast(frag, kf), qf[ks], s);
        }
        // ---- band and tail mask, selected: key(r) = tk0 + 32kb + 4h + (r & 3) + 8 (r >> 2).  SP: the list's validity mask in
        // the band test's place, a bit per key(r)
        if constexpr (SP) {
            const unsigned mh = kb ? (unsigned)(m_cur >> 32) : (unsigned)m_cur;  // this wave's key block (uniform)
            if (mh != 0xffffffffu) {
                const unsigned mv = mh >> (4 * h);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (!((mv >> ((r & 3) + 8 * (r >> 2))) & 1)) s[r] = -INFINITY;
            }
        } else if (tk0 < lo_max || tk0 + kBC - 1 > hi_min) {
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
        __syncthreads();
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
            s[r] = p;
            rs += p;
        }
        lsum = lsum * coeff + rs;
        // registers 8ss .. 8ss + 7 are the B fragment of k-step 2kb + ss for this row, half h
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            frag pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (T)s[8 * ss + j];  // RTNE
            *(LDS_PTR(u32x4))(lds + p_wr + 32 * ss) = __builtin_bit_cast(u32x4, pf);
        }
        if (kb == 0 && h == 0) cf[32 * rb + i] = coeff;
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
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const frag p0 = __builtin_bit_cast(frag, *(LDS_PTR(u32x4))(lds + p_rd + 32 * ks));
            const frag p1 = __builtin_bit_cast(frag, *(LDS_PTR(u32x4))(lds + p_rd + 32 * kPRowB + 32 * ks));
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const s16x4 vlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + ks * 16 * kRowB + v_off[0][db]));
                const s16x4 vhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + ks * 16 * kRowB + v_off[1][db]));
                const frag vf = __builtin_bit_cast(frag, (s16x8)__builtin_shufflevector(vlo, vhi, 0, 1, 2, 3, 4, 5, 6, 7));
                o[db][0] = M::mfma(vf, p0, o[db][0]);
                o[db][1] = M::mfma(vf, p1, o[db][1]);
            }
        }
        __syncthreads();  // every read of this step's tile and of P has retired
        if (more) stage_write();
        m_cur = m_nxt;
        __syncthreads();
    }

    // ---- the rows' sums and maxima to the P.V lanes
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
        const int ediv = row / (VT ? a.g : N_q);  // (recomputed, not carried from the S phase: no register lives across the loop)
        const int erem = row - ediv * (VT ? a.g : N_q);
        const int hg = VT ? erem : ediv;
        const int qi = VT ? ediv : erem;
        const int head = hk * a.g + hg;
        const float l = xl[32 * rbp + i] + xl[64 + 32 * rbp + i];
        const float mr = mf[32 * rbp + i];
        const bool seen = l > 0.0f;
        float inv = seen ? 1.0f / l : 0.0f;
        if constexpr (F8) inv = seen ? inv * vd : 0.0f;  // O = vd (P V8) / l, in fp32
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
            if (wave == 0 && h == 0) {
                T *lp = (T *)a.L + b * a.ls[0] + head * a.ls[1] + start + qi;
                *lp = seen ? (T)(mr + __builtin_amdgcn_logf(l)) : (T)INFINITY;
            }
        } else {
            // (SP: the rows of all B * N_q positions, this one's position `start`)
            const int64_t rows = VQ ? (int64_t)a.total_q * a.H : (int64_t)(SP ? spB : gridDim.z) * a.H * (SP ? a.N_q : N_q);
            const int64_t prow = (int64_t)split * rows + (VQ   ? (int64_t)(start + qi) * a.H + head
                                                          : SP ? ((int64_t)b * a.H + head) * a.N_q + start
                                                               : ((int64_t)b * a.H + head) * N_q + qi);
            float *op = a.o_part + prow * kDV + 128 * wave + 4 * h;
            float invp = inv;
            // SP, VQ: the products of this branch are kept apart from the one-split branch's.  The compiler otherwise hoists a product
            // the two branches share above them, and the one-split branch then rounds that fp32 product to f16 (two roundings) where
            // the fixed dense kernel's v_fma_mixlo_f16 rounds once: one ulp of one element in some 10^5, against the bit-for-bit tests
            if constexpr (SP || VQ) asm volatile("" : "+v"(invp));
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

constexpr bool kVQ = FA2_DECODE_VARLEN_Q != 0, kSP = FA2_DECODE_SPARSE != 0;

template <typename T, typename C, bool PAGED> int launch_t(const Fa2DecodeProblem &p, const DecodeMlaArgs &a) {
    // (the lists: one position a workgroup, over B * N_q positions or, packed, total_q rows)
    const long long gx = (long long)p.num_splits * a.row_tiles * (kSP ? (kVQ ? (long long)p.total_q : (long long)p.B * p.N_q) : 1);
    if (gx > 0x7fffffffLL) {
        fa2_set_error(kSP && kVQ ? "kvcache mla sparse varlen: grid too large (total_q * num_splits * head tiles = %lld)"
                      : kSP      ? "kvcache mla sparse: grid too large (B * N_q * num_splits * head tiles = %lld)"
                          : "kvcache mla16 kernel: grid too large (num_splits * row tiles = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    static Fa2DeviceLatch attr_done;  // more than 64 KiB of dynamic LDS: opt in, once per device
    if (attr_done.need()) {
        (void)hipFuncSetAttribute((const void *)fa2_decode_mla16_kernel<T, C, PAGED, kVQ, kSP>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem);
        attr_done.mark();
    }
    const dim3 grid((unsigned)gx, p.H_kv, kSP ? 1 : p.B), block(256);
    hipLaunchKernelGGL((fa2_decode_mla16_kernel<T, C, PAGED, kVQ, kSP>), grid, block, kSmem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache mla16 kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <typename T, typename C> int launch_p(const Fa2DecodeProblem &p, const DecodeMlaArgs &a) {
    return p.table ? launch_t<T, C, true>(p, a) : launch_t<T, C, false>(p, a);
}

template <typename T> int launch_c(const Fa2DecodeProblem &p, const DecodeMlaArgs &a) {
    if (p.kv_dtype == FA2_DTYPE_F8E4M3) return launch_p<T, CacheE4M3>(p, a);
    if (p.kv_dtype == FA2_DTYPE_F8E5M2) return launch_p<T, CacheE5M2>(p, a);
    return launch_p<T, T>(p, a);
}

bool fp8_cache(const Fa2DecodeProblem &p) { return p.kv_dtype == FA2_DTYPE_F8E4M3 || p.kv_dtype == FA2_DTYPE_F8E5M2; }

bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

// (packed queries: N_q holds max_seqlen_q, so the row bound below is the grid's)
bool supports(const Fa2DecodeProblem &p) {
    if (!fa2_decode_mla16_shape(p.d, p.d_v, p.dtype) || (p.kv_dtype != p.dtype && !fp8_cache(p)) || (p.cu_q != nullptr) != kVQ ||
        (p.indices != nullptr) != kSP)
        return false;
    if (p.V != p.K) return false;  // the value operand is read from K's LDS image
    for (int k = 0; k < 4; ++k)
        if (p.vs[k] != p.ks[k]) return false;
    if (!(p.scale > 0.0f) || !(p.scale < INFINITY)) return false;
    if (!kSP && (int64_t)(p.H / p.H_kv) * p.N_q > (1 << 24)) return false;  // (rows of a KV group are counted in 32 bits)
    if (p.qs[3] != 1 || p.ks[3] != 1 || p.os[3] != 1) return false;
    // 16-byte vector loads of Q and K rows, 8-byte stores of O: every row start must stay aligned (an fp8 cache: 16 elements)
    const int64_t kmask = fp8_cache(p) ? 15 : 7;
    for (int k = 0; k < 3; ++k)
        if ((p.qs[k] & 7) || (p.ks[k] & kmask) || (p.os[k] & 7)) return false;
    if (!aligned16(p.Q) || !aligned16(p.K) || !aligned16(p.O)) return false;
    if (p.num_splits > 1 && !aligned16(p.o_part)) return false;
    // paged: a 64-key tile must lie inside one page; the block stride is ks[0] above
    if (!kSP && p.table && p.page_size % FA2_KVCACHE_KEY_TILE != 0) return false;  // (a list addresses every row on its own)
    return true;
}

int launch(const Fa2DecodeProblem &p) {
    if (!supports(p)) {
        fa2_set_error("kvcache mla16 kernel: needs f16/bf16, d = 576 and d_v = 512, V aliasing K (the same pointer and strides), unit "
                      "d-stride, 16-byte aligned rows (and workspace), scale > 0%s%s",
                      fp8_cache(p) ? "; an fp8 cache: every stride of K a multiple of 16 elements and a 16-byte aligned base" : "",
                      p.table && !kSP ? ", page_size % 64 == 0 for a paged cache (other page sizes: the generic kernel)" : "");
        return FA2_ERR_UNSUPPORTED;
    }
    DecodeMlaArgs a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K;
    a.O = (char *)p.O; a.L = (char *)p.L;
    const int64_t cb = fp8_cache(p) ? 1 : 2;  // bytes per cache element
    for (int k = 0; k < 3; ++k) { a.qs[k] = p.qs[k] * 2; a.ks[k] = p.ks[k] * cb; a.os[k] = p.os[k] * 2; }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.seqlens = p.seqlens;
    a.H = p.H; a.g = p.H / p.H_kv; a.N_q = p.N_q; a.S_k = p.S_k; a.causal = p.causal; a.wl = p.wl; a.wr = p.wr;
    a.num_splits = p.num_splits;
    a.row_tiles = (int)(((int64_t)a.g * (kSP ? 1 : p.N_q) + 63) / 64);
    a.o_part = p.o_part; a.l_part = p.l_part;
    a.c_log2e = (float)((double)p.scale * FA2_LOG2E);
    a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.kd = p.kd; a.vd = p.vd;
    for (int k = 0; k < 2; ++k) { a.kds[k] = p.kds[k]; a.vds[k] = p.vds[k]; }
    a.cu_q = p.cu_q; a.total_q = p.total_q;
#if FA2_DECODE_SPARSE
    a.idx = p.indices; a.topk = p.topk; a.B = p.B;
    for (int k = 0; k < 4; ++k) a.is[k] = p.is[k];
#endif
    return p.dtype == FA2_DTYPE_BF16 ? launch_c<__bf16>(p, a) : launch_c<_Float16>(p, a);
}

}  // namespace

#if FA2_DECODE_SPARSE && FA2_DECODE_VARLEN_Q
bool fa2_decode_mla16_sv_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mla16_sv(const Fa2DecodeProblem &p) { return launch(p); }
#elif FA2_DECODE_SPARSE
bool fa2_decode_mla16_s_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mla16_s(const Fa2DecodeProblem &p) { return launch(p); }
#elif FA2_DECODE_VARLEN_Q
bool fa2_decode_mla16_v_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mla16_v(const Fa2DecodeProblem &p) { return launch(p); }
#else
bool fa2_decode_mla16_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mla16(const Fa2DecodeProblem &p) { return launch(p); }
#endif
