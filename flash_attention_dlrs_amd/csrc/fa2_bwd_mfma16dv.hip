// fa2_bwd_mfma16dv.hip -- packed FA-2 backward for f16 / bf16 with a value head size of its own, d = 192 / d_v = 128 (un-absorbed MLA
// prefill: fa2_bwd_varlen_dv), on v_mfma_f32_32x32x16_{bf16,f16}.
//
// The varlen GQA form of fa2_bwd_mfma16.hip written out for this one shape: the same arithmetic, the same two owner launches (the
// query owner first, handing L + log2(rowsum P) in fp32 through the second half of D), nothing summed across workgroups, the GQA
// group sum inside one key-owner workgroup in fixed order, fa2_varlen_seq / fa2_varlen_band with block skips and masks on both band
// edges, LDS-DMA staging with the swizzle through the source address, P shared from the dV wave to the dK wave through LDS.
//
// What differs: the two swept tiles no longer have one width, and neither do the owned fragment sets.
//   T0 (Q in the key-owner launch, K in the query-owner launch) is 192 wide and staged as the forward's two images
//   (fa2_mfma16dv.hip): image A = columns 0..127 in the d = 128 layout (lds_off<128>), image B = columns 128..191 in the d = 64
//   layout (lds_off<64>, source offset + 256 B).  Row reads: k-steps 0..7 on A, 8..11 on B; transposed reads: output column blocks
//   0..3 from A, 4..5 from B.  T1 (dO or V) is 128 wide: the d = 128 image unchanged.
//   Key owner: ONE owned-fragment array of 8 -- V in a dK wave (it computes dP and reads P from the slot), K's k-steps 0..7 in a dV
//   wave (it computes S) -- and ONE accumulator array of 6 blocks, of which a dV wave accumulates into 4 and keeps K's k-steps 8..11
//   as the bits of the fifth: two waves per SIMD.
//   Query owner: Q (12) and dO (8) fragments beside 96 dQ^T accumulators do not fit 256 registers with the rest: one wave per SIMD
//   (__launch_bounds__(256, 1)), the parent's code with wider arrays.
#include "fa2_bwd_common.h"
#include "fa2_mfma.h"

namespace {

struct VArgs {
    const char *Q, *K, *V, *O, *dO, *L;
    char *dQ, *dK, *dV;
    float *D;
    int64_t qs[3], ks[3], vs[3], os[3], dos[3], dqs[3], dks[3], dvs[3];  // (unused), H, token strides in BYTES
    int64_t ls[2];                                                        // elements
    int B, H, gqa, vcausal;
    int wl, wr;  // raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    const int32_t *cu_q, *cu_k;
    int max_q, max_k, total_q, total_k;
    float c_log2e, scale;
};

constexpr int BS = 64;                       // swept rows per tile
constexpr int IMGA = BS * 256, IMGB = BS * 128;  // the two images of a 192-wide tile
constexpr int TILEW = IMGA + IMGB, TILEN = BS * 256;
constexpr int NOFF = 2 * TILEW;              // LDS: T0[2] (A | B each) | T1[2] | L[2][64] | D[2][64] | P slots (key owner only)
constexpr int LOFF = NOFF + 2 * TILEN;
constexpr int POFF = LOFF + 4 * BS * 4;      // P slots: [4 key groups][2][4 KiB]
constexpr int KS0 = 12, KS1 = 8;             // k-steps of a product over d / over d_v
constexpr int DB0 = 6, DB1 = 4;              // 32-column output blocks of a 192- / 128-wide gradient

// ---- D[h, token] = sum_x O * dO over the d_v = 128 columns: 16 lanes per row, 16 bytes of each operand per lane
template <typename T> __global__ __launch_bounds__(256) void bwd_D_dv_kernel(const VArgs a) {
    constexpr int LPR = 16;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = gid / LPR, rows = (long long)a.H * a.total_q;
    const int ch = (int)(gid % LPR);
    float s = 0.0f;
    if (r < rows) {
        const int n = (int)(r % a.total_q), h = (int)(r / a.total_q);
        typedef __attribute__((ext_vector_type(8))) T Tx8;
        const Tx8 o = *(const Tx8 *)(a.O + h * a.os[1] + (int64_t)n * a.os[2] + ch * 16);
        const Tx8 g = *(const Tx8 *)(a.dO + h * a.dos[1] + (int64_t)n * a.dos[2] + ch * 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (float)o[j] * (float)g[j];
    }
#pragma unroll
    for (int w = 1; w < LPR; w <<= 1) s += __shfl_xor(s, w, 64);
    if (r < rows && ch == 0) a.D[r] = s;
}

// MODE 0: key owner (dK, dV), 8 waves.  MODE 1: query owner (dQ), 4 waves.
template <typename T, int MODE>
__global__ __launch_bounds__(MODE == 0 ? 512 : 256, MODE == 0 ? 2 : 1) void bwd_mfma16dv_kernel(const VArgs a) {
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr int NW = MODE == 0 ? 8 : 4, BO = 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int N = MODE == 0 ? a.max_k : a.max_q;  // (only the block count: the sequence's own extents are NO and NS)
    int wl = 0, wr = 0;
    auto band_none = [&](int q0, int q1, int k0, int k1) { return k0 > q1 + wr || k1 < q0 - wl; };
    auto band_all = [&](int q0, int q1, int k0, int k1) { return k0 >= q1 - wl && k1 <= q0 + wr; };

    const int HO = MODE == 0 ? a.H / a.gqa : a.H;  // heads of the grid: MODE 0 KV heads, MODE 1 query heads
    const int nblk = (N + BO - 1) / BO, nbh = a.B * HO;
    int bh, blk;
    {
        const int bid = blockIdx.x;
        if ((nbh & 7) == 0) {  // whole (b, h) groups per XCD (speed only)
            const int slot = bid >> 3;
            bh = (slot / nblk) * 8 + (bid & 7);
            blk = slot % nblk;
        } else {
            bh = bid / nblk;
            blk = bid % nblk;
        }
    }
    const int b = bh / HO, hh = bh - b * HO;     // hh: MODE 0 the KV head, MODE 1 the query head
    const int hk = MODE == 0 ? hh : hh / a.gqa;  // the KV head
    int qst, NQ, kst, NK;
    fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, qst, NQ);
    fa2_varlen_seq(a.cu_k, b, a.total_k, a.max_k, kst, NK);
    qst = __builtin_amdgcn_readfirstlane(qst);
    NQ = __builtin_amdgcn_readfirstlane(NQ);
    kst = __builtin_amdgcn_readfirstlane(kst);
    NK = __builtin_amdgcn_readfirstlane(NK);
    const int NO = MODE == 0 ? NK : NQ, NS = MODE == 0 ? NQ : NK;
    if (blk * BO >= NO) return;  // (whole workgroup, before any barrier)
    fa2_varlen_band(NQ, NK, a.vcausal, a.wl, a.wr, wl, wr);

    const bool roleV = MODE == 0 && wave >= 4;  // MODE 0: waves 4..7 accumulate dV^T, waves 0..3 dK^T
    if (MODE == 0 && roleV) __builtin_amdgcn_s_setprio(1);  // the dV waves carry the exp2 work (fa2_bwd_mfma16.hip)
    const int own0 = blk * BO + (MODE == 0 ? wave & 3 : wave) * 32;  // first owned row of this wave
    const int orow = own0 + i;                                       // this lane's owned row

    // this lane's output row, formed here and held in two registers: the epilogue then needs none of the scalars above, which would
    // otherwise stay live (and spill) across the sweep
    char *op;
    {
        char *base = MODE == 1 ? a.dQ : (roleV ? a.dV : a.dK);
        const int64_t *st = MODE == 1 ? a.dqs : (roleV ? a.dvs : a.dks);
        op = base + (int64_t)(MODE == 1 ? qst : kst) * st[2] + hh * st[1] + (int64_t)orow * st[2] + h * 8;  // (MODE 0: hh = hk)
        if (orow >= NO) op = nullptr;  // (rows past the owned extent store nothing)
        asm volatile("" : "+v"(op));
    }
    const char *Ks = a.K + (int64_t)kst * a.ks[2] + hk * a.ks[1], *Vs = a.V + (int64_t)kst * a.vs[2] + hk * a.vs[1];
    const int64_t t0rs = MODE == 1 ? a.ks[2] : a.qs[2], t1rs = MODE == 1 ? a.vs[2] : a.dos[2];

    f32x16 acc0[DB0];  // dQ^T (MODE 1), dK^T (MODE 0, waves 0..3) or dV^T in its first four blocks (MODE 0, waves 4..7)
#pragma unroll
    for (int db = 0; db < DB0; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[db][r] = 0.0f;

    // ---- owned fragments.  MODE 1: f0 = Q (12), f1 = dO (8).  MODE 0: f0 alone, 8 wide -- V in a dK wave; in a dV wave K's k-steps
    // 0..7, and K's k-steps 8..11 (16 registers) as the bits of accumulator block 4, which a dV wave never accumulates into: the
    // register file is allocated per kernel, and this way neither role carries registers only the other one uses.
    frag f0[MODE == 1 ? KS0 : KS1], f1[MODE == 1 ? KS1 : 1];
    auto f0_at = [&](int ks) __attribute__((always_inline)) {  // the owned first-product fragment of k-step ks
        if (MODE == 1 || ks < KS1) return f0[MODE == 1 ? ks : ks & 7];
        const int e = 4 * (ks - KS1);
        const f32x4 v = {acc0[4][e], acc0[4][e + 1], acc0[4][e + 2], acc0[4][e + 3]};
        return __builtin_bit_cast(frag, v);
    };
    float Lown = 0.0f, Down = 0.0f;  // MODE 1: the owned query's L and D
    {
        const int row = orow < NO ? orow : NO - 1;
        if (MODE == 1) {
            const char *p0 = a.Q + (int64_t)qst * a.qs[2] + hh * a.qs[1] + (int64_t)row * a.qs[2] + h * 16;
            const char *p1 = a.dO + (int64_t)qst * a.dos[2] + hh * a.dos[1] + (int64_t)row * a.dos[2] + h * 16;
#pragma unroll
            for (int ks = 0; ks < KS0; ++ks) f0[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(p0 + ks * 32));
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) f1[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(p1 + ks * 32));
            Lown = (float)((const T *)a.L + hh * a.ls[1] + qst)[row];
            Down = (a.D + (int64_t)hh * a.total_q + qst)[row];
        } else if (roleV) {
            const char *p0 = Ks + (int64_t)row * a.ks[2] + h * 16;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) f0[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(p0 + ks * 32));
#pragma unroll
            for (int ks = KS1; ks < KS0; ++ks) {
                const f32x4 v = __builtin_bit_cast(f32x4, *(const u32x4 *)(p0 + ks * 32));
#pragma unroll
                for (int j = 0; j < 4; ++j) acc0[4][4 * (ks - KS1) + j] = v[j];
            }
        } else {
            const char *p1 = Vs + (int64_t)row * a.vs[2] + h * 16;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) f0[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(p1 + ks * 32));
        }
    }
    // the owned fragments must have landed before the sweep: the compiler's counted waits inside the loop would also wait for the
    // LDS-DMA pieces it cannot see (fa2_bwd_mfma16.hip)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched

    float rsum = 0.0f;  // MODE 1: this lane's share of rowsum(P) of its query
    const float c = a.c_log2e;

    // ---- what does not depend on the query head: the staging pattern and the read offsets
    // staging by LDS-DMA in 1 KiB pieces, wave w issues pieces w, w + NW, ...: image A and T1 hold 4 rows per piece (16 pieces), image
    // B 8 rows per piece (8 pieces); lane l of a piece fills LDS (row, slot) with global chunk slot ^ swz(row)
    // (a wave's next piece lies 4 NW or 8 NW rows on, a multiple of 16: the same swizzle, a scalar step in the source offset)
    constexpr int PPA = 16 / NW, PPB = 8 / NW;
    int soA, soN, soB;
    {
        const int row = 4 * wave + lane / 16, chunk = (lane % 16) ^ swz<128>(row);
        soA = row * (int)t0rs + chunk * 16;
        soN = row * (int)t1rs + chunk * 16;
        const int rowb = 8 * wave + lane / 8, chunkb = (lane % 8) ^ swz<64>(rowb);
        soB = rowb * (int)t0rs + 256 + chunkb * 16;
    }
    auto make_rsrc = [&](const char *base, int bytes) {
        const uint64_t ba = (uint64_t)base;
        i32x4 r;
        r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)ba);
        r[1] = __builtin_amdgcn_readfirstlane((int)((uint32_t)(ba >> 32) & 0xffffu));
        r[2] = __builtin_amdgcn_readfirstlane(bytes);
        r[3] = 0x00020000;
        return r;
    };
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds);

    // Read offsets inside a tile, all from four per-lane bases: a 32-row block starts at a multiple of 4 KiB and the bases stay below
    // it, and a k-step or column block only flips chunk bits the swizzle XORs into -- chunk 2 ks + h = (2 ks) ^ h, column block db adds
    // 4 db to the chunk, rows + 8 flip chunk bit 1 -- so every offset is (block + base) ^ constant: one VALU operation per read in place
    // of 24 registers of offsets, which the key-owner launch does not have.
    const int w_ = (lane >> 4) & 1, qq_ = (lane >> 2) & 3, pp_ = lane & 3;
    const int kb0 = lds_off<128>(i, h), kb1 = lds_off<64>(i, h);  // row reads: row i of the block, chunk 2 ks + h (image A / T1, image B)
    // transposed reads (fa2_mfma16.hip): rows 4 h + qq (+ 8 u) of the 16-row k-step, chunk 4 db + 2 w + (pp >> 1)
    const int vb0 = lds_off<128>(4 * h + qq_, 2 * w_ + (pp_ >> 1)) + 8 * (pp_ & 1), vb1 = lds_off<64>(4 * h + qq_, 2 * w_ + (pp_ >> 1)) + 8 * (pp_ & 1);
    auto row_read = [&](int blk_off, int base, int ks) __attribute__((always_inline)) {
        return *(LDS_PTR(u32x4))(lds + ((blk_off + base) ^ (ks << 5)));
    };
    // one A fragment of T^T: rows 16 ss .. + 15 of the block, column block db; UROW = the byte distance of 8 rows
    auto tr_read = [&](int blk_off, int base, int db, int urow) __attribute__((always_inline)) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + ((blk_off + base) ^ (db << 6))));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + ((blk_off + base) ^ ((db << 6) | urow | 32))));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    // acc[0..5] += T0^T . B over the 32 swept rows of block kb of buffer cur (blocks 0..3 from image A, 4..5 from image B)
    auto second_wide = [&](int cur, int kb, const f32x16 &x) __attribute__((always_inline)) {
        const int tA = cur * TILEW + kb * 32 * 256, tB = cur * TILEW + IMGA + kb * 32 * 128;
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            frag bf;
#pragma unroll
            for (int j = 0; j < 8; ++j) bf[j] = (T)x[8 * ss + j];  // RTNE casts of kernels.py:293 / :317
#pragma unroll
            for (int db = 0; db < DB0; ++db) {
                const s16x8 tf = db < 4 ? tr_read(tA + ss * 16 * 256, vb0, db, 8 * 256) : tr_read(tB + ss * 16 * 128, vb1, db - 4, 8 * 128);
                acc0[db] = M::mfma(__builtin_bit_cast(frag, tf), bf, acc0[db]);
            }
        }
    };

    const int wg0 = blk * BO;
    int t_begin, t_end;
    {  // MODE 1 sweeps the keys [i0 - wl, i1 + wr], MODE 0 the queries [j0 - wr, j1 + wl]
        const int lo = wg0 - (MODE == 1 ? wl : wr), hi = wg0 + BO - 1 + (MODE == 1 ? wr : wl);
        t_begin = (lo > 0 ? lo : 0) / BS;
        t_end = (NS == 0 || hi < 0) ? 0 : (hi < NS - 1 ? hi : NS - 1) / BS + 1;  // (nothing to sweep: no swept row, or all before 0)
        if (t_begin >= t_end) t_begin = t_end;
    }

    const int ngq = MODE == 0 ? a.gqa : 1;
    for (int gq = 0; gq < ngq; ++gq) {  // MODE 0: the group's query heads in order; MODE 1: its own head, once
        const int hq = MODE == 0 ? hk * a.gqa + gq : hh;
        const char *T0p = MODE == 1 ? Ks : a.Q + (int64_t)qst * a.qs[2] + hq * a.qs[1];
        const char *T1p = MODE == 1 ? Vs : a.dO + (int64_t)qst * a.dos[2] + hq * a.dos[1];
        const float *Dp = a.D + (int64_t)hq * a.total_q + qst;
        float *Lc = a.D + (int64_t)a.H * a.total_q + (int64_t)hq * a.total_q + qst;
        // (NS = 0: an empty range -- every load reads 0, and nothing is swept)
        const i32x4 rs0 = make_rsrc(T0p, NS > 0 ? (NS - 1) * (int)t0rs + 384 : 0);
        const i32x4 rs1 = make_rsrc(T1p, NS > 0 ? (NS - 1) * (int)t1rs + 256 : 0);
        const i32x4 rsL = make_rsrc((const char *)Lc, NS * 4), rsD = make_rsrc((const char *)Dp, NS * 4);  // (MODE 0: NS = NQ)
        auto stage_load = [&](int t) {  // the target buffer t & 1 must be free when this is called
            // (the buffer and the tile's row offset stay scalars the compiler cannot fold ahead of time: it would otherwise keep the first
            // tile's per-lane offsets and LDS targets of every piece in registers across the sweep of the previous query head)
            int buf = t & 1, r0 = t * BS * (int)t0rs, r1 = t * BS * (int)t1rs;
            asm volatile("" : "+s"(buf), "+s"(r0), "+s"(r1));
#pragma unroll
            for (int pp = 0; pp < PPA; ++pp) {
                dma16(rs0, lds_base + buf * TILEW + (wave + pp * NW) * 1024, soA + (r0 + pp * 4 * NW * (int)t0rs));
                dma16(rs1, lds_base + NOFF + buf * TILEN + (wave + pp * NW) * 1024, soN + (r1 + pp * 4 * NW * (int)t1rs));
            }
#pragma unroll
            for (int pp = 0; pp < PPB; ++pp)
                dma16(rs0, lds_base + buf * TILEW + IMGA + (wave + pp * NW) * 1024, soB + (r0 + pp * 8 * NW * (int)t0rs));
            if (MODE == 0 && wave == 0) {
                dma4(rsL, lds_base + LOFF + buf * BS * 4, (t * BS + lane) * 4);
                dma4(rsD, lds_base + LOFF + (2 * BS + buf * BS) * 4, (t * BS + lane) * 4);
            }
        };

        if (t_begin < t_end) {
            stage_load(t_begin);
            dma_wait();
        }
        __syncthreads();

        if constexpr (MODE == 0) {
            // ---- key-owner launch: the dV wave and the dK wave of a key group (waves kg + 4 and kg: one SIMD) share P through LDS; the
            // dK wave runs one 32-row block behind (fa2_bwd_mfma16.hip).  Per block: dV wave 12 + 8 MFMAs, dK wave 8 + 12.
            const int kg = wave & 3;
            auto blk_skip = [&](int bidx) { return band_none(bidx * 32, bidx * 32 + 31, own0, own0 + 31); };
            auto blk_masked = [&](int bidx) { return (bidx * 32 + 32 > NS) || !band_all(bidx * 32, bidx * 32 + 31, own0, own0 + 31); };
            for (int sidx = 2 * t_begin; sidx <= 2 * t_end; ++sidx) {
                const int t = sidx >> 1, kb = sidx & 1;
                // tile t+1 goes into the buffer of tile t-1, which the dK waves still read in the kb == 0 step
                if (kb == 1 && t + 1 < t_end) stage_load(t + 1);
                const int bidx = roleV ? sidx : sidx - 1;  // the block this wave works on in this step
                const bool work = roleV ? sidx < 2 * t_end : sidx - 1 >= 2 * t_begin;
                if (work && !blk_skip(bidx)) {
                    const int cur = (bidx >> 1) & 1, kbb = bidx & 1, srow0 = bidx * 32;
                    const int slot = POFF + (kg * 2 + (bidx & 1)) * 4096 + lane * 16;
                    f32x16 x;
#pragma unroll
                    for (int r = 0; r < 16; ++r) x[r] = 0.0f;
                    if (roleV) {
                        const int tA = cur * TILEW + kbb * 32 * 256, tB = cur * TILEW + IMGA + kbb * 32 * 128;
#pragma unroll
                        for (int ks = 0; ks < KS0; ++ks) {
                            const u32x4 qf = ks < 8 ? row_read(tA, kb0, ks) : row_read(tB, kb1, ks - 8);
                            x = M::mfma(__builtin_bit_cast(frag, qf), f0_at(ks), x);  // kernels.py:283 (without the log2e factor)
                        }
                        auto pbody = [&](auto masked_) __attribute__((always_inline)) {
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                const f32x4 lv = *(LDS_PTR(f32x4))(lds + LOFF + (cur * BS + kbb * 32 + 8 * g + 4 * h) * 4);
                                f32x4 pv;
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(x[4 * g + j], c, -lv[j]));  // :285
                                    if (decltype(masked_)::value) {
                                        const int qry = srow0 + 8 * g + 4 * h + j;
                                        if (qry >= NS || orow < qry - wl || orow > qry + wr) pe = 0.0f;
                                    }
                                    pv[j] = pe;
                                    x[4 * g + j] = pe;
                                }
                                *(LDS_PTR(f32x4))(lds + slot + g * 1024) = pv;
                            }
                        };
                        if (blk_masked(bidx)) pbody(IC<1>{});  // one wave-uniform branch, two straight-line bodies
                        else pbody(IC<0>{});
                        // dV^T += dO^T P: the dO tile, 4 column blocks
                        const int tN = NOFF + cur * TILEN + kbb * 32 * 256;
#pragma unroll
                        for (int ss = 0; ss < 2; ++ss) {
                            frag bf;
#pragma unroll
                            for (int j = 0; j < 8; ++j) bf[j] = (T)x[8 * ss + j];  // RTNE cast of :287
#pragma unroll
                            for (int db = 0; db < DB1; ++db) {
                                const s16x8 tf = tr_read(tN + ss * 16 * 256, vb0, db, 8 * 256);
                                acc0[db] = M::mfma(__builtin_bit_cast(frag, tf), bf, acc0[db]);
                            }
                        }
                    } else {
                        const int tN = NOFF + cur * TILEN + kbb * 32 * 256;
#pragma unroll
                        for (int ks = 0; ks < KS1; ++ks) {
                            const u32x4 gf = row_read(tN, kb0, ks);
                            x = M::mfma(__builtin_bit_cast(frag, gf), f0[ks], x);  // :289 (f0 holds V here)
                        }
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 dv = *(LDS_PTR(f32x4))(lds + LOFF + (2 * BS + cur * BS + kbb * 32 + 8 * g + 4 * h) * 4);
                            const f32x4 pv = *(LDS_PTR(f32x4))(lds + slot + g * 1024);
#pragma unroll
                            for (int j = 0; j < 4; ++j) x[4 * g + j] = pv[j] * (x[4 * g + j] - dv[j]);  // :291
                        }
                        second_wide(cur, kbb, x);  // dK^T += Q^T dS
                    }
                }
                if (kb == 1 && t + 1 < t_end) dma_wait();
                __syncthreads();
            }
        } else {
            for (int t = t_begin; t < t_end; ++t) {
                const int cur = t & 1;
                const bool more = t + 1 < t_end;
                if (more) stage_load(t + 1);
                if (!band_none(own0, own0 + 31, t * BS, t * BS + BS - 1)) {
#pragma nounroll
                    for (int kb = 0; kb < 2; ++kb) {
                        const int srow0 = t * BS + kb * 32;  // first key of this 32-key block
                        if (band_none(own0, own0 + 31, srow0, srow0 + 31)) continue;
                        f32x16 x0, x1;
#pragma unroll
                        for (int r = 0; r < 16; ++r) x0[r] = x1[r] = 0.0f;
                        const int tA = cur * TILEW + kb * 32 * 256, tB = cur * TILEW + IMGA + kb * 32 * 128;
                        const int tN = NOFF + cur * TILEN + kb * 32 * 256;
#pragma unroll
                        for (int ks = 0; ks < KS0; ++ks) {
                            const u32x4 kf = ks < 8 ? row_read(tA, kb0, ks) : row_read(tB, kb1, ks - 8);
                            x0 = M::mfma(__builtin_bit_cast(frag, kf), f0_at(ks), x0);  // kernels.py:283: S^T = K Q^T (without the log2e factor)
                        }
                        // dP^T = V dO^T (8 MFMAs) with P = exp2(c S - L) of the finished S tile underneath, two elements per MFMA, one
                        // step behind (fa2_bwd_mfma16.hip)
#pragma unroll
                        for (int ks = 0; ks < KS1; ++ks) {
                            const u32x4 vf = row_read(tN, kb0, ks);
                            x1 = M::mfma(__builtin_bit_cast(frag, vf), f1[ks], x1);  // :289
                            if (ks >= 1) {
#pragma unroll
                                for (int e = 0; e < 2; ++e) {
                                    const int r = (ks - 1) * 2 + e;
                                    x0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(x0[r], c, -Lown));  // :285
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int r = (KS1 - 1) * 2 + e;
                            x0[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(x0[r], c, -Lown));
                        }
                        // key of register r: srow0 + (r & 3) + 8 (r >> 2) + 4 h
                        const bool need_mask = (srow0 + 32 > NS) || !band_all(own0, own0 + 31, srow0, srow0 + 31);
                        auto body = [&](auto masked_) __attribute__((always_inline)) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                float p = x0[r];
                                if (decltype(masked_)::value) {
                                    const int key = srow0 + 8 * (r >> 2) + 4 * h + (r & 3);
                                    if (key >= NS || key < orow - wl || key > orow + wr) p = 0.0f;
                                }
                                rsum += p;
                                x1[r] = p * (x1[r] - Down);  // :291 (the scale factor is applied once, at the end)
                            }
                        };
                        if (need_mask) body(IC<1>{});
                        else body(IC<0>{});
                        second_wide(cur, kb, x1);  // dQ^T += K^T dS^T
                    }
                }
                if (more) dma_wait();
                __syncthreads();
            }
        }
    }  // gq: every sweep ends on a barrier, so the next head's first tile may take either buffer

    // ---- epilogue: lane (i, h) owns output row `orow` (op), columns 32 db + 8 g + 4 h .. + 3
    const float tot = MODE == 1 ? half_swap_sum(rsum) : 1.0f;  // lanes i and i + 32 share a query
    if (op) {
        auto store_rows = [&](int ndb, float mul) __attribute__((always_inline)) {
#pragma unroll
            for (int db = 0; db < DB0; ++db) {
                if (db >= ndb) break;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    typedef __attribute__((ext_vector_type(4))) T Tx4;
                    Tx4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (T)(acc0[db][4 * g + j] * mul);
                    *(u32x2 *)(op + db * 64 + g * 16) = __builtin_bit_cast(u32x2, v);
                }
            }
        };
        if (MODE == 1) {
            // a query without a visible key: rowsum 0, dQ 0, and the statistic stays +inf (not inf + log2(0))
            store_rows(DB0, tot > 0.0f ? a.scale / tot : 0.0f);
            if (h == 0) (a.D + (int64_t)a.H * a.total_q + (int64_t)hh * a.total_q + qst)[orow] = tot > 0.0f ? Lown + __builtin_amdgcn_logf(tot) : INFINITY;
        } else if (!roleV) {
            store_rows(DB0, a.scale);
        } else {
            store_rows(DB1, 1.0f);
        }
    }
}

constexpr size_t kSmem1 = LOFF, kSmem0 = POFF + 4 * 2 * 4096;  // 80 KiB, 113 KiB

template <typename T> int launch_t(const Fa2BwdProblem &p, const VArgs &a) {
    // D over every packed token; each mode's grid from its own owned extent (MODE 1: max_q, MODE 0: max_k)
    const long long lanes = (long long)p.H * p.total_q * 16;
    if (lanes > 0) hipLaunchKernelGGL((bwd_D_dv_kernel<T>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, p.stream, a);
    const long long nblkq = (long long)((p.max_q + 127) / 128) * p.B * p.H, nblk = (long long)((p.max_k + 127) / 128) * p.B * (p.H / a.gqa);
    if (nblkq > 0x7fffffffLL || nblk > 0x7fffffffLL) {
        fa2_set_error("backward mfma16dv: grid too large");
        return FA2_ERR_BAD_ARG;
    }
    static Fa2DeviceLatch attr_set;  // > 64 KiB of dynamic LDS needs the attribute; once per instantiation
    if (attr_set.need()) {
        (void)hipFuncSetAttribute((const void *)bwd_mfma16dv_kernel<T, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmem1);
        (void)hipFuncSetAttribute((const void *)bwd_mfma16dv_kernel<T, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmem0);
        attr_set.mark();
    }
    if (nblkq > 0)  // first: it leaves the fp32 row statistic the key-owner launch reads
        hipLaunchKernelGGL((bwd_mfma16dv_kernel<T, 1>), dim3((unsigned)nblkq), dim3(256), kSmem1, p.stream, a);
    if (nblk > 0) hipLaunchKernelGGL((bwd_mfma16dv_kernel<T, 0>), dim3((unsigned)nblk), dim3(512), kSmem0, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("backward mfma16dv launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

}  // namespace

bool fa2_bwd_mfma16dv_supports(const Fa2BwdProblem &p) {
    if (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16) return false;
    if (p.d != 192 || p.dv != 128) return false;
    if (!(p.scale > 0.0f) || !(p.scale < INFINITY)) return false;
    const int64_t *all[8] = {p.qs, p.ks, p.vs, p.os, p.dos, p.dqs, p.dks, p.dvs};
    for (int t = 0; t < 8; ++t) {
        if (all[t][3] != 1) return false;
        for (int k = 0; k < 3; ++k)
            if (all[t][k] & 7) return false;  // 16-byte vector accesses of whole rows
    }
    const void *ptrs[8] = {p.Q, p.K, p.V, p.O, p.dO, p.dQ, p.dK, p.dV};
    for (int t = 0; t < 8; ++t)
        if ((uintptr_t)ptrs[t] & 15) return false;
    if (p.N > (1 << 24)) return false;
    // 32-bit buffer offsets of the LDS-DMA staging: (N + 64) rows of every swept tensor below 2 GiB (N: the longer max_seqlen)
    for (int t = 0; t < 5; ++t)
        if ((int64_t)(p.N + 64) * all[t][2] * 2 >= (1LL << 31)) return false;
    return true;
}

int fa2_bwd_launch_mfma16dv(const Fa2BwdProblem &p, int gqa) {
    if (!fa2_bwd_mfma16dv_supports(p)) {
        fa2_set_error("backward mfma16dv: needs f16/bf16, d = 192 and d_v = 128, unit d-stride, 16-byte aligned rows, scale > 0");
        return FA2_ERR_UNSUPPORTED;
    }
    VArgs a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K; a.V = (const char *)p.V; a.O = (const char *)p.O;
    a.dO = (const char *)p.dO; a.L = (const char *)p.L;
    a.dQ = (char *)p.dQ; a.dK = (char *)p.dK; a.dV = (char *)p.dV; a.D = (float *)p.D;
    for (int k = 0; k < 3; ++k) {
        a.qs[k] = p.qs[k] * 2; a.ks[k] = p.ks[k] * 2; a.vs[k] = p.vs[k] * 2; a.os[k] = p.os[k] * 2;
        a.dos[k] = p.dos[k] * 2; a.dqs[k] = p.dqs[k] * 2; a.dks[k] = p.dks[k] * 2; a.dvs[k] = p.dvs[k] * 2;
    }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.B = p.B; a.H = p.H; a.gqa = gqa;
    a.vcausal = p.causal ? 1 : 0;
    a.wl = p.wl; a.wr = p.wr;
    a.cu_q = p.cu_q; a.cu_k = p.cu_k; a.max_q = p.max_q; a.max_k = p.max_k; a.total_q = p.total_q; a.total_k = p.total_k;
    a.c_log2e = (float)((double)p.scale * FA2_LOG2E);
    a.scale = p.scale;
    return p.dtype == FA2_DTYPE_BF16 ? launch_t<__bf16>(p, a) : launch_t<_Float16>(p, a);
}
