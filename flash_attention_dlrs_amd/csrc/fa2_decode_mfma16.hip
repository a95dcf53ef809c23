// fa2_decode_mfma16.hip -- KV-cache decode for f16 / bf16, d in {64, 128} (fa2_fwd_kvcache and fa2_fwd_kvcache_fp8,
// FA2_KVCACHE_VARIANT_MFMA16): the flash-decoding structure on the matrix cores, over a 16-bit or an fp8 cache.
//
// One workgroup of four waves handles one (b, KV head, split).  The g = H / H_kv query heads of the group times the N_q query
// positions are the R = g N_q <= 64 rows of the tile's query side (row r = head-in-group * N_q + query; padded to 32 or 64, the
// padding rows computed and dropped), so every K and V byte of the group is read from HBM once, not once per query head.  The
// waves take DIFFERENT keys of the split: with RB = ceil(R / 32) row blocks the workgroup has KG = 4 / RB key groups, and key
// group k owns the BC-key tiles t = k (mod KG) of the split.  Each wave runs the tile loop of fa2_mfma16k.hip on its tiles --
// S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_32x32x16, exp2-domain online softmax, P rounded to the I/O dtype -- and at the end
// key groups 1.. hand their (m, l, O) to group 0 through LDS, merged as two key tiles are.
//
// Staging.  All 256 threads load the KG tiles of a step with 16-byte row-contiguous loads into registers while the waves
// compute on the tiles of the previous step in LDS (single-buffered: 64 KiB per workgroup at most, two workgroups per CU, so
// 128 KiB of loads are in flight per CU).  Addresses are built in 64 bits per thread: no 32-bit offset limit on S_k x stride.
//
// Stale cache contents.  A chunk of a key >= the split's end (<= N_k(b)) is not loaded: it is written to LDS as zeros, for K
// and for V (0 x NaN in the P.V MFMA would be NaN), and its score is SELECTED to -inf.  So what lies behind cache_seqlens[b]
// is never read.
//
// fp8 cache (fa2_fwd_kvcache_fp8).  The cache element type C is a template parameter: T itself, or OCP e4m3fn / e5m2 with
// per-(b, h_kv) descales kd, vd.  Only staging differs: a thread's 16-byte load holds 16 elements, v_cvt_scalef32_pk_* at scale
// 1.0 converts them (exactly: both formats are subsets of f16 and of bf16) to two 16-byte chunks, which land in LDS chunks 2c and
// 2c + 1 of the same swizzle.  The descales are folded, not applied per element: kd into the softmax scale of the workgroup, vd
// into the fp32 normalisation of the output, before it is rounded or written as a partial.  A chunk past the split's end is
// zeros before the conversion, so no stale byte (NaN and inf patterns included) is ever converted.
//
// Paged cache (fa2_fwd_kvcache_paged).  PAGED is a template parameter as well: K and V are a page pool and key j of sequence b
// is row j % page_size of page table[b][j / page_size].  Only the tile's base address differs.  With page_size % 64 == 0 a key
// tile (32 or 64 keys on a multiple of its size) lies inside one page, so its table entry is uniform over the workgroup:
// stage_load reads it with one scalar load per tile, clamps it to [0, num_blocks - 1] (a wild entry gives a wrong result, never
// an access outside the pool) and folds it into the tile's 64-bit base.  The load for step s + 1 is issued a compute step ahead
// of its use, as the tile's own loads are.  The entry of a tile at or past the split's end is not loaded.
//
// Output.  num_splits == 1: O / l and L = m + log2 l in the I/O dtype, a row without a visible key as O = 0, L = +inf.
// Otherwise every (split, row) writes the normalised fp32 partial O_s and L_s (an empty split: 0 and -inf) for the combine
// launch (fa2_decode_combine.hip); vector stores only.
//
// Variable-length queries (fa2_fwd_kvcache_varlen).  VQ is a template parameter too, instantiated in fa2_decode_mfma16_v.hip
// (FA2_DECODE_VARLEN_Q) alone: Q and O are packed (total_q, H, d), sequence b owns n_q(b) rows (fa2_varlen_seq), and a workgroup
// owns tq = min(64 / g, max_seqlen_q) consecutive query positions [q0, q1) of one sequence for the g heads of the group: row
// r = head-in-group * tq + (position - q0), R = g tq <= 64.  The grid's x axis is (split, query tile); a tile at or past n_q(b)
// leaves at once.  The mask is the band of n_q(b) and N_k(b), the row's position counted in the SEQUENCE; the key range of
// the split is clipped to the band of the tile's own rows [q0, q1), whole 64-key tiles outside it neither loaded nor looked up.
// Rows at positions >= n_q(b) are computed and dropped: in the packed layout they would be the next sequence's.  With VQ false
// q0 = 0, q1 = tq = N_q and every expression below is the fixed-N_q kernel's.
#include "fa2_decode.h"
#include "fa2_mfma.h"

#ifndef FA2_DECODE_VARLEN_Q
#define FA2_DECODE_VARLEN_Q 0
#endif

namespace {

// (the cache element types other than T, CacheE4M3 / CacheE5M2, and their exact conversion CacheCvt: fa2_decode.h)

struct DecodeMfmaArgs {
    const char *Q, *K, *V;
    char *O, *L;
    int64_t qs[3], ks[3], vs[3], os[3];  // B, H, N strides in BYTES (d stride is 1 element)
    int64_t ls[2];                       // L strides in elements
    const int32_t *seqlens;
    int H, g, N_q, S_k, causal, wl, wr, num_splits;
    float *o_part, *l_part;
    float c_log2e;  // scale * log2(e) > 0
    const float *kd, *vd;  // fp8 cache only: descales at [b * kds[0] + h_kv * kds[1]], null = 1
    int64_t kds[2], vds[2];
    const int32_t *table;  // paged cache only: entry [b, i] at b * table_stride + i; ks[0], vs[0] are the block strides
    int64_t table_stride;
    int page_size, num_blocks;
    const int32_t *cu_q;  // VQ only: B + 1 offsets into the packed rows; qs[0] = os[0] = ls[0] = 0
    int total_q, max_q, tq, nqt;  // nqt = ceil(max_q / tq) query tiles per (split, KV head, sequence)
};

// RB = 32-row blocks of the query side, KG = key groups (RB * KG = 4 waves), BC = keys per tile (32 or 64).  C: the cache
// element type, T or CacheE4M3 / CacheE5M2.  PAGED: K and V are a page pool behind a block table.  VQ: packed queries, tiled.
template <typename T, typename C, bool PAGED, bool VQ, int D, int RB, int KG, int BC>
__global__ __launch_bounds__(RB * KG * 64, 2) void fa2_decode_mfma16_kernel(const DecodeMfmaArgs a) {
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr bool F8 = !__is_same(C, T);
    constexpr int NT = RB * KG * 64;
    constexpr int ROWB = D * 2, TILEB = BC * ROWB;  // of the 16-bit LDS tile
    constexpr int GROWB = F8 ? D : ROWB;            // bytes of a cache row in memory
    constexpr int CPR = GROWB / 16, CPT = BC * CPR / NT;  // 16-byte loads per row, per thread and tile
    constexpr int RPI = NT / CPR;  // tile rows covered per staging pass
    constexpr int KS = D / 16, DB = D / 32, KB = BC / 32;
    constexpr int GRPB = 2 * TILEB;  // LDS per key group: K | V
    static_assert(RPI % 16 == 0 && CPT >= 1 && CPT * RPI == BC, "staging passes must tile the key tile in multiples of 16 rows");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rb = wave % RB, grp = wave / RB;
    const int i = lane & 31, h = lane >> 5;
    const int hk = blockIdx.y, b = blockIdx.z;
    // N_q: the query count of the mask; TQ: query positions of the tile, [q0, q1) the ones it owns, from packed row `start` on
    int split = blockIdx.x, N_q = a.N_q, TQ = a.N_q, q0 = 0, start = 0;
    if constexpr (VQ) {
        split = blockIdx.x / a.nqt;
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, start, N_q);
        TQ = a.tq;
        q0 = (blockIdx.x - split * a.nqt) * TQ;
        if (q0 >= N_q) return;  // no rows: nothing to write, no partials
    }
    const int q1 = VQ ? (q0 + TQ < N_q ? q0 + TQ : N_q) : N_q;
    const int R = a.g * TQ;

    int NK, k0, k1;
    fa2_decode_split(a.seqlens, b, a.S_k, a.num_splits, split, NK, k0, k1);
    int wl, wr;
    fa2_varlen_band(N_q, NK, a.causal, a.wl, a.wr, wl, wr);
    // the keys of the split that the band of any row of the tile touches: [kb0, ke), kb0 on a 64-key boundary (the rest is skipped)
    const int lo_t = q0 - wl;                              // the first key the tile's first row sees
    const int lo_min = lo_t > k0 ? (lo_t & ~63) : k0;  // (k0 is a multiple of 64)
    const int kb0 = lo_min > k0 ? lo_min : k0;
    const int hi_end = q1 + wr;  // one past the last key the last row sees
    const int ke = hi_end < k1 ? hi_end : k1;
    const int nt = ke > kb0 ? (ke - kb0 + BC - 1) / BC : 0;
    const int nstep = (nt + KG - 1) / KG;

    // ---- this lane's row: (head of the group, query position); padding rows repeat the last row and are not stored
    const int row = rb * 32 + i;
    const int rowc = row < R ? row : R - 1;
    const int hg = rowc / TQ;
    int qi = q0 + rowc - hg * TQ;  // position in the sequence
    bool keep = row < R;
    if constexpr (VQ) {  // positions past the sequence's last: the last row again, dropped
        keep = keep && qi < N_q;
        qi = qi < N_q ? qi : N_q - 1;
    }
    const int head = hk * a.g + hg;

    // ---- Q fragments: B operand of S^T = K Q^T.  Lane (i, h) holds Q[row][16ks + 8h .. +7].
    frag qf[KS];
    {
        const char *qp = a.Q + b * a.qs[0] + head * a.qs[1] + (int64_t)(start + qi) * a.qs[2] + h * 16;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(qp + ks * 32));
    }

    // ---- staging map: thread handles chunk (row = it*RPI + tid/CPR, ch = tid%CPR) of each tile.
    const int st_row = tid / CPR, st_ch = tid % CPR;
    // (paged: the page and the tile's first row in it are the tile's, added in stage_load)
    const char *kg = a.K + hk * a.ks[1] + (PAGED ? (int64_t)st_row * a.ks[2] : b * a.ks[0] + (int64_t)(kb0 + st_row) * a.ks[2]) + st_ch * 16;
    const char *vg = a.V + hk * a.vs[1] + (PAGED ? (int64_t)st_row * a.vs[2] : b * a.vs[0] + (int64_t)(kb0 + st_row) * a.vs[2]) + st_ch * 16;
    // + it*RPI*ROWB (swizzle depends on row&15 only).  fp8: the load's 16 elements are LDS chunks 2 st_ch and 2 st_ch + 1.
    const int st_lds = lds_off<D>(st_row, F8 ? 2 * st_ch : st_ch);
    const int st_lds1 = F8 ? lds_off<D>(st_row, 2 * st_ch + 1) : 0;

    // paged: the walk over the pages.  stage_load takes the tiles in order (g inside s, s = 0, 1, ...), a tile is BC keys on a
    // multiple of BC and page_size is a multiple of 64: (pg_i, pg_row) -- the page of the next tile and the tile's first row in it
    // -- advance by BC rows per tile and wrap at page_size, all in scalar registers, no division in the loop.
    static_assert(!PAGED || FA2_KVCACHE_KEY_TILE % BC == 0, "a key tile must not straddle a page");
    int pg_i = 0, pg_row = 0;
    const int32_t *tab = nullptr;
    if constexpr (PAGED) {
        pg_i = kb0 / a.page_size;
        pg_row = kb0 - pg_i * a.page_size;
        tab = a.table + b * a.table_stride;
    }
    u32x4 kreg[KG][CPT], vreg[KG][CPT];
    auto stage_load = [&](int s) {
#pragma unroll
        for (int g = 0; g < KG; ++g) {
            int64_t kpage = 0, vpage = 0;  // paged: byte offset of the tile's first row from the pool's (hk, row 0)
            if constexpr (PAGED) {
                // one scalar load per tile; the entry of a tile at or past the split's end (<= N_k) is not part of the problem and
                // may lie past the table's row: not loaded (every chunk of such a tile is zeros below)
                if (kb0 + (KG * s + g) * BC < ke) {
                    const int64_t e = fa2_decode_page(tab, pg_i, a.num_blocks);
                    kpage = e * a.ks[0] + (int64_t)pg_row * a.ks[2];
                    vpage = e * a.vs[0] + (int64_t)pg_row * a.vs[2];
                }
                pg_row += BC;
                if (pg_row >= a.page_size) {
                    pg_row = 0;
                    ++pg_i;
                }
            }
#pragma unroll
            for (int it = 0; it < CPT; ++it) {
                const int rel = (KG * s + g) * BC + it * RPI;  // tile row 0 of this pass, relative to kb0
                const bool ok = kb0 + rel + st_row < ke;       // past the split's end (<= N_k): zeros, never read
                const int64_t ko = PAGED ? kpage + (int64_t)(it * RPI) * a.ks[2] : (int64_t)rel * a.ks[2];
                const int64_t vo = PAGED ? vpage + (int64_t)(it * RPI) * a.vs[2] : (int64_t)rel * a.vs[2];
                kreg[g][it] = ok ? *(const u32x4 *)(kg + ko) : u32x4{0, 0, 0, 0};
                vreg[g][it] = ok ? *(const u32x4 *)(vg + vo) : u32x4{0, 0, 0, 0};
            }
        }
    };
    auto stage_write = [&]() {
#pragma unroll
        for (int g = 0; g < KG; ++g)
#pragma unroll
            for (int it = 0; it < CPT; ++it) {
                if constexpr (F8) {  // word j of the load = elements 4j .. 4j + 3 = words 2j, 2j + 1 of the 16-bit row
                    using X = CacheCvt<T, C>;
#pragma unroll
                    for (int kv = 0; kv < 2; ++kv) {
                        const u32x4 w = kv ? vreg[g][it] : kreg[g][it];
                        const u32x4 lo = {X::template cvt<false>(w[0]), X::template cvt<true>(w[0]), X::template cvt<false>(w[1]),
                                          X::template cvt<true>(w[1])};
                        const u32x4 hi = {X::template cvt<false>(w[2]), X::template cvt<true>(w[2]), X::template cvt<false>(w[3]),
                                          X::template cvt<true>(w[3])};
                        *(LDS_PTR(u32x4))(lds + g * GRPB + kv * TILEB + st_lds + it * RPI * ROWB) = lo;
                        *(LDS_PTR(u32x4))(lds + g * GRPB + kv * TILEB + st_lds1 + it * RPI * ROWB) = hi;
                    }
                } else {
                    *(LDS_PTR(u32x4))(lds + g * GRPB + st_lds + it * RPI * ROWB) = kreg[g][it];
                    *(LDS_PTR(u32x4))(lds + g * GRPB + TILEB + st_lds + it * RPI * ROWB) = vreg[g][it];
                }
            }
    };

    // ---- per-lane LDS read offsets (fa2_mfma16k.hip): K row read: row kb*32 + i, chunk 2ks + h; V transposed read
    // (ds_read_b64_tr_b16): lane 4q+p of a 16-lane group supplies row (base + 4h + q), columns 32db + 16(group&1) + 4p..+3.
    int k_off[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) k_off[ks] = grp * GRPB + lds_off<D>(i, 2 * ks + h);
    int v_off[2][DB];
    {
        const int w = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int db = 0; db < DB; ++db)
                v_off[u][db] = grp * GRPB + TILEB + lds_off<D>(8 * u + 4 * h + qq, 4 * db + 2 * w + (pp >> 1)) + 8 * (pp & 1);
    }

    f32x16 o[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
    float m = -INFINITY, lsum = 0.0f;
    // fp8: one scalar load per descale and workgroup.  S = (scale kd) Q K8^T; vd waits in a scalar register for the epilogue.
    float c = a.c_log2e, vd = 1.0f;
    if constexpr (F8) {
        c *= fa2_decode_descale(a.kd, a.kds[0], a.kds[1], b, hk);
        vd = fa2_decode_descale(a.vd, a.vds[0], a.vds[1], b, hk);
    }
    // this row's visible keys [lo, hi], and whether a tile can meet a band edge of any row
    const int lo = qi - wl, hi = (qi + wr) < (ke - 1) ? (qi + wr) : (ke - 1);
    const int lo_max = q1 - 1 - wl, hi_min = (q0 + wr) < (ke - 1) ? (q0 + wr) : (ke - 1);

    if (nstep > 0) {
        stage_load(0);
        stage_write();
    }
    __syncthreads();

    for (int st = 0; st < nstep; ++st) {
        const bool more = st + 1 < nstep;
        if (more) stage_load(st + 1);

        const int t = KG * st + grp;  // this wave's key tile of the step
        if (t < nt) {
            const int tk0 = kb0 + t * BC;
            // ---- S^T = K . Q^T : KB 32-key blocks.
            f32x16 s[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4 kf = *(LDS_PTR(u32x4))(lds + kb * 32 * ROWB + k_off[ks]);
                    s[kb] = M::mfma(__builtin_bit_cast(frag, kf), qf[ks], s[kb]);
                }
            }
            // ---- band and tail mask, selected: key(kb, r) = tk0 + 4h + kb*32 + (r&3) + 8*(r>>2)
            if (tk0 < lo_max || tk0 + BC - 1 > hi_min) {
                const int kl = lo - (tk0 + 4 * h), kh = hi - (tk0 + 4 * h);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kb * 32 + (r & 3) + 8 * (r >> 2);
                        if (key < kl || key > kh) s[kb][r] = -INFINITY;
                    }
            }
            // ---- online softmax, one query row per lane pair (i, h).  While a row's maximum is -inf (no visible key so far) P
            // and the rescale factor are 0, not exp2(-inf + inf).
            float mx = s[0][0];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx * c);
            const float m_use = m_new == -INFINITY ? 0.0f : m_new;
            const float coeff = __builtin_amdgcn_exp2f(m - m_use);
            m = m_new;
            float rs = 0.0f;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][r], c, -m_use));
                    s[kb][r] = p;
                    rs += p;
                }
            lsum = lsum * coeff + rs;
            if (__any(coeff != 1.0f)) {
#pragma unroll
                for (int db = 0; db < DB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[db][r] *= coeff;
            }
            // ---- O^T += V^T . P^T.  k-step (kb, ss) = keys kb*32 + 16ss .. +15; registers 8ss..8ss+7 of s[kb] are the B fragment.
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int ss = 0; ss < 2; ++ss) {
                    frag pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (T)s[kb][8 * ss + j];  // RTNE
                    const int rowb = (kb * 32 + ss * 16) * ROWB;
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const s16x4 vlo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + rowb + v_off[0][db]));
                        const s16x4 vhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + rowb + v_off[1][db]));
                        const s16x8 vf = __builtin_shufflevector(vlo, vhi, 0, 1, 2, 3, 4, 5, 6, 7);
                        o[db] = M::mfma(__builtin_bit_cast(frag, vf), pf, o[db]);
                    }
                }
        }
        __syncthreads();  // every read of this step's tiles has retired
        if (more) stage_write();
        __syncthreads();
    }

    // ---- merge of the key groups: waves of groups 1.. hand (O, m, l) to the wave of group 0 with their row block through LDS
    // ([register][lane] floats; the loop's last barrier has retired every read of the K/V tiles), combined like key tiles.
    if constexpr (KG > 1) {
        constexpr int NREG = DB * 16 + 2;
        static_assert((KG - 1) * RB * NREG * 256 <= KG * GRPB, "exchange area exceeds the K/V buffers");
        if (grp > 0) {
            LDS_PTR(float) xch = (LDS_PTR(float))lds + ((grp - 1) * RB + rb) * NREG * 64 + lane;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) xch[(db * 16 + r) * 64] = o[db][r];
            xch[(DB * 16) * 64] = m;
            xch[(DB * 16 + 1) * 64] = lsum;
        }
        __syncthreads();
        if (grp > 0) return;
#pragma unroll
        for (int g = 1; g < KG; ++g) {
            LDS_PTR(float) xch = (LDS_PTR(float))lds + ((g - 1) * RB + rb) * NREG * 64 + lane;
            const float m1 = xch[(DB * 16) * 64], l1 = xch[(DB * 16 + 1) * 64];
            const float mm = fmaxf(m, m1);
            const float mu = mm == -INFINITY ? 0.0f : mm;  // both groups without a visible key: factors 0, not NaN
            const float a0 = __builtin_amdgcn_exp2f(m - mu), a1 = __builtin_amdgcn_exp2f(m1 - mu);
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] = o[db][r] * a0 + xch[(db * 16 + r) * 64] * a1;
            lsum = lsum * a0 + l1 * a1;
            m = mm;
        }
    }

    // ---- epilogue.  Lane (i, h) owns its row, columns 32db + 8g + 4h .. +3 for g = 0..3.
    const float l = lsum + __shfl_xor(lsum, 32, 64);
    const bool seen = l > 0.0f;
    float inv = seen ? 1.0f / l : 0.0f;
    if constexpr (F8) inv = seen ? inv * vd : 0.0f;  // O = vd (P V8) / l, in fp32
    if (!keep) return;
    if (a.num_splits == 1) {
        char *op = a.O + b * a.os[0] + head * a.os[1] + (int64_t)(start + qi) * a.os[2] + h * 8;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                typedef __attribute__((ext_vector_type(4))) T Tx4;
                Tx4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (T)(o[db][4 * g + j] * inv);
                *(u32x2 *)(op + db * 64 + g * 16) = __builtin_bit_cast(u32x2, v);
            }
        if (h == 0) {
            T *lp = (T *)a.L + b * a.ls[0] + head * a.ls[1] + start + qi;
            *lp = seen ? (T)(m + __builtin_amdgcn_logf(l)) : (T)INFINITY;
        }
    } else {
        const int64_t rows = VQ ? (int64_t)a.total_q * a.H : (int64_t)gridDim.z * a.H * N_q;
        const int64_t prow = (int64_t)split * rows + (VQ ? (int64_t)(start + qi) * a.H + head : ((int64_t)b * a.H + head) * N_q + qi);
        float *op = a.o_part + prow * D + h * 4;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = o[db][4 * g + j] * inv;
                *(f32x4 *)(op + db * 32 + g * 8) = v;
            }
        if (h == 0) a.l_part[prow] = seen ? m + __builtin_amdgcn_logf(l) : -INFINITY;
    }
}

constexpr bool kVQ = FA2_DECODE_VARLEN_Q != 0;

template <typename T, typename C, bool PAGED, int D, int RB, int KG, int BC> int launch_t(const Fa2DecodeProblem &p, const DecodeMfmaArgs &a) {
    const long long gx = kVQ ? (long long)p.num_splits * a.nqt : p.num_splits;
    if (gx > 0x7fffffffLL) {
        fa2_set_error("kvcache mfma16 kernel: grid too large (num_splits * query tiles = %lld)", gx);
        return FA2_ERR_BAD_ARG;
    }
    const dim3 grid((unsigned)gx, p.H_kv, p.B), block(RB * KG * 64);
    constexpr size_t smem = (size_t)KG * 2 * BC * D * 2;
    static_assert(smem <= 64 * 1024, "two workgroups per CU");
    hipLaunchKernelGGL((fa2_decode_mfma16_kernel<T, C, PAGED, kVQ, D, RB, KG, BC>), grid, block, smem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache mfma16 kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <typename T, typename C, bool PAGED> int launch_d(const Fa2DecodeProblem &p, const DecodeMfmaArgs &a) {
    const bool one = (int64_t)a.g * (kVQ ? a.tq : p.N_q) <= 32;  // one 32-row block: four key groups
    if (p.d == 128) return one ? launch_t<T, C, PAGED, 128, 1, 4, 32>(p, a) : launch_t<T, C, PAGED, 128, 2, 2, 64>(p, a);
    return one ? launch_t<T, C, PAGED, 64, 1, 4, 64>(p, a) : launch_t<T, C, PAGED, 64, 2, 2, 64>(p, a);
}

template <typename T, typename C> int launch_p(const Fa2DecodeProblem &p, const DecodeMfmaArgs &a) {
    return p.table ? launch_d<T, C, true>(p, a) : launch_d<T, C, false>(p, a);
}

template <typename T> int launch_c(const Fa2DecodeProblem &p, const DecodeMfmaArgs &a) {
    if (p.kv_dtype == FA2_DTYPE_F8E4M3) return launch_p<T, CacheE4M3>(p, a);
    if (p.kv_dtype == FA2_DTYPE_F8E5M2) return launch_p<T, CacheE5M2>(p, a);
    return launch_p<T, T>(p, a);
}

bool fp8_cache(const Fa2DecodeProblem &p) { return p.kv_dtype == FA2_DTYPE_F8E4M3 || p.kv_dtype == FA2_DTYPE_F8E5M2; }

bool aligned16(const void *q) { return ((uintptr_t)q & 15) == 0; }

// (packed queries: the tile holds 64 / g positions, so only g itself is bounded)
bool supports(const Fa2DecodeProblem &p) {
    if (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16) return false;
    if (p.kv_dtype != p.dtype && !fp8_cache(p)) return false;
    if (p.d != 64 && p.d != 128) return false;
    if (!(p.scale > 0.0f) || !(p.scale < INFINITY)) return false;
    if ((int64_t)(p.H / p.H_kv) * (kVQ ? 1 : p.N_q) > 64) return false;
    if (p.qs[3] != 1 || p.ks[3] != 1 || p.vs[3] != 1 || p.os[3] != 1) return false;
    // 16-byte vector loads of Q/K/V rows, 8-byte stores of O: every row start must stay aligned (an fp8 cache: 16 elements).
    const int64_t kmask = fp8_cache(p) ? 15 : 7;
    for (int k = 0; k < 3; ++k)
        if ((p.qs[k] & 7) || (p.ks[k] & kmask) || (p.vs[k] & kmask) || (p.os[k] & 7)) return false;
    if (!aligned16(p.Q) || !aligned16(p.K) || !aligned16(p.V) || !aligned16(p.O)) return false;
    if (p.num_splits > 1 && !aligned16(p.o_part)) return false;
    // paged: a key tile (32 or 64 keys on a multiple of its size) must lie inside one page; the block stride is ks[0] above
    if (p.table && p.page_size % FA2_KVCACHE_KEY_TILE != 0) return false;
    return true;
}

int launch(const Fa2DecodeProblem &p) {
    if (!supports(p)) {
        fa2_set_error("kvcache mfma16 kernel: needs f16/bf16 (the cache alike, or fp8), d in {64,128}, %s <= 64, unit d-stride, "
                      "16-byte aligned rows (and workspace), scale > 0%s", kVQ ? "g = H / H_kv" : "g * N_q",
                      p.table ? ", page_size % 64 == 0 for a paged cache (other page sizes: the generic kernel)" : "");
        return FA2_ERR_UNSUPPORTED;
    }
    DecodeMfmaArgs a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K; a.V = (const char *)p.V;
    a.O = (char *)p.O; a.L = (char *)p.L;
    const int64_t cb = fp8_cache(p) ? 1 : 2;  // bytes per cache element
    for (int k = 0; k < 3; ++k) {
        a.qs[k] = p.qs[k] * 2; a.ks[k] = p.ks[k] * cb; a.vs[k] = p.vs[k] * cb; a.os[k] = p.os[k] * 2;
    }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.seqlens = p.seqlens;
    a.H = p.H; a.g = p.H / p.H_kv; a.N_q = p.N_q; a.S_k = p.S_k; a.causal = p.causal; a.wl = p.wl; a.wr = p.wr;
    a.num_splits = p.num_splits;
    a.o_part = p.o_part; a.l_part = p.l_part;
    a.c_log2e = (float)((double)p.scale * FA2_LOG2E);
    a.kd = p.kd; a.vd = p.vd;
    for (int k = 0; k < 2; ++k) { a.kds[k] = p.kds[k]; a.vds[k] = p.vds[k]; }
    a.table = p.table; a.table_stride = p.table_stride; a.page_size = p.page_size; a.num_blocks = p.num_blocks;
    a.cu_q = p.cu_q; a.total_q = p.total_q; a.max_q = p.max_q;
    a.tq = kVQ ? fa2_decode_varlen_tq(a.g, p.max_q) : p.N_q;
    a.nqt = kVQ ? (p.max_q + a.tq - 1) / a.tq : 1;
    return p.dtype == FA2_DTYPE_BF16 ? launch_c<__bf16>(p, a) : launch_c<_Float16>(p, a);
}

}  // namespace

#if FA2_DECODE_VARLEN_Q
bool fa2_decode_mfma16_v_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mfma16_v(const Fa2DecodeProblem &p) { return launch(p); }
#else
bool fa2_decode_mfma16_supports(const Fa2DecodeProblem &p) { return supports(p); }
int fa2_launch_decode_mfma16(const Fa2DecodeProblem &p) { return launch(p); }
#endif
