// fa2_mfma16d_kernel.h -- the software-pipelined f16 / bf16 kernel of fa2_mfma16p.hip with LDS-DMA staging
// (variant "mfma16d").  Same arithmetic (src/flash_attention_kernels.py:84-108), same 32-key block schedule
// (QK^T of block j+1 under the softmax of block j), same K-unit / V-tile scheme; what changes is how a tile
// gets from HBM/L2 into LDS: `buffer_load_dwordx4 ... lds` writes 1 KiB per wave-instruction straight into
// LDS -- no staging registers, no ds_write_b128 (ablation of fa2_mfma16p.hip: its LDS writes cost ~11 %).
//
// LDS-DMA writes lane-linearly (M0 base + lane * 16), so rows cannot be padded: the tile image is plain
// 256-byte (d = 128) or 128-byte (d = 64) rows with the 16-byte chunks XOR-swizzled THROUGH THE SOURCE
// ADDRESS (the lane that fills (row, slot) fetches global chunk slot ^ f(row)) and the same XOR on every read.
// f is the involution swz() of lds_off() (fa2_mfma.h): conflict-free for the ds_read_b128 row reads of K and for
// the ds_read_b64_tr_b16 transposed reads of V.  Rows past N (and the "negative" rows of K unit 0) are
// zero-filled by the buffer descriptor's range check.
#pragma once
#include "fa2_common.h"
#include "fa2_mfma.h"

//
// One kernel template serves every attention form: the form is the last template parameter F, a set of the bits of fa2_common.h, and
// each form's statements stand in an `if constexpr` branch of their own (merged into shared expressions they are scheduled
// differently: keep them apart).  F = 0 is the plain kernel.  The launchers in fa2_mfma16d.hip name the five sets that exist.
//   kWindow: local attention -- key j visible to query i iff i - wl <= j <= i + wr, one tile per workgroup, the key loop from the
//            64-key unit of the tile's first visible key, blocks outside a wave's band skipped, blocks across its edges masked.
//   kVarlen (with kWindow): the variable-length form -- one tile of ceil(max_q / BR) per workgroup and sequence; the workgroup reads
//            its sequence's offsets, leaves when its tile starts past the sequence's queries, and runs the windowed loop with the
//            query extent NQ, the key extent NK and the bottom-right shifted band (fa2_varlen_band).  Base pointers are built in
//            64 bits from the sequence starts, so the 32-bit buffer offsets only span one sequence.  A row without a visible key
//            gets O = 0 and L = +inf.
//   kGqa (with kWindow): grouped-query attention -- K and V have H / gqa heads and query head hh reads KV head hh / gqa.
//
// The 48 instantiations compile in two translation units, split by element type so that neither is the longest compile of the
// build: fa2_mfma16d.hip (bf16) and fa2_mfma16d_f16.hip (f16, behind launch_f16).

namespace fa2_mfma16d {

struct DmaArgs {
    const char *Q, *K, *V;
    char *O, *L;
    int64_t qs[3], ks[3], vs[3], os[3];  // B, H, N strides in bytes
    int64_t ls[2];
    int B, H, N;
    float c_log2e;
    int group;
    int flags;  // experiment switches (FA2_FLAGS): 1 = static priority for waves 4..7
    // the forms' fields, behind the plain kernel's (whose offsets they leave alone); 0 where a form does not use them
    // kWindow: window sides, normalised to [0, N - 1] (fa2_window_normalise)
    // kVarlen: raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    int wl, wr;
    int causal;  // kVarlen: the causal flag of the band
    const int32_t *cu_q, *cu_k;
    int max_q, max_k, total_q, total_k;
    int gqa;  // kGqa: query heads per KV head
};

template <typename T, int D, int NW, bool CAUSAL, int F = 0>
__global__ __launch_bounds__(NW * 64, 2) void fa2_fwd_mfma16d_kernel(const DmaArgs a) {
    using M = Mma<T>;
    using frag = typename M::frag;
    constexpr int BR = NW * 32;
    constexpr int ROWB = D * 2, CPR = ROWB / 16;   // bytes per row, 16-byte chunks per row
    constexpr int TILEB = 64 * ROWB;               // K unit = V tile = 64 rows
    constexpr int RPP = 1024 / ROWB;               // rows per 1-KiB DMA piece (4 or 8)
    constexpr int PIECES = TILEB / 1024, PPW = PIECES / NW;  // pieces per tile, per wave
    constexpr int VBASE = 2 * TILEB;               // LDS: Kunit0 | Kunit1 | Vtile0 | Vtile1
    constexpr int KS = D / 16, DB = D / 32;
    static_assert(PPW >= 1, "too many waves for this tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (M0, scalar branches)
    const int i = lane & 31, h = lane >> 5;
    // N: the extent the tiles are counted over; NQ and NK: the query and key extents (kVarlen: the sequence's own, set below)
    const int N = F & kVarlen ? a.max_q : a.N;
    int qst = 0, NQ = N, kst = 0, NK = N, wl = 0, wr = 0;
    if constexpr ((F & (kWindow | kVarlen)) == kWindow) {
        wl = a.wl;
        wr = a.wr;
    }
    // T5 static form (cdna_hip_programming.md): the second-dispatched half loses VALU arbitration on every segment
    if ((a.flags & 1) && wave >= NW / 2) __builtin_amdgcn_s_setprio(1);

    // Causal: a workgroup owns the PAIR of Q tiles (nq-1-p, p) of one (b, h) and runs them back to back, heavy one
    // first -- every workgroup then does the same amount of work (nq+1 tile-steps), so the 256 CUs finish together
    // instead of trailing off through the light tiles; the pair shares its K/V through L2.  Non-causal: one tile.
    const int nq = (N + BR - 1) / BR, nbh = a.B * a.H;
    const int nunit = CAUSAL ? (nq + 1) / 2 : nq;  // work units (tile pairs / tiles) per (b, h)
    int bh, unit;
    {
        const int bid = blockIdx.x;
        if ((nbh & 7) == 0) {  // whole (b, h) groups per XCD (speed only)
            const int slot = bid >> 3, G = a.group;
            const int batch = slot / (G * nunit), r = slot - batch * (G * nunit);
            bh = (batch * G + r % G) * 8 + (bid & 7);
            unit = r / G;
        } else {
            bh = bid / nunit;
            unit = bid % nunit;
        }
    }
    const int qi_first = CAUSAL ? nq - 1 - unit : unit, qi_second = unit;
    const int npass = (CAUSAL && qi_second != qi_first) ? 2 : 1;
    const int b = bh / a.H, hh = bh - b * a.H;
    int q0 = 0, qrow = 0;  // set per pass

    if constexpr (F & kVarlen) {
        fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, qst, NQ);
        fa2_varlen_seq(a.cu_k, b, a.total_k, a.max_k, kst, NK);
        qst = __builtin_amdgcn_readfirstlane(qst);
        NQ = __builtin_amdgcn_readfirstlane(NQ);
        kst = __builtin_amdgcn_readfirstlane(kst);
        NK = __builtin_amdgcn_readfirstlane(NK);
        if (qi_first * BR >= NQ) return;  // (whole workgroup, before any barrier)
        fa2_varlen_band(NQ, NK, a.causal, a.wl, a.wr, wl, wr);
    }
    const int hk = F & kGqa ? hh / a.gqa : hh;  // the KV head
    // kVarlen: bases from the sequence starts (token stride in qs[2], ...)
    const char *Qp = F & kVarlen ? a.Q + (int64_t)qst * a.qs[2] + (int64_t)hh * a.qs[1]
                                 : a.Q + (int64_t)b * a.qs[0] + (int64_t)hh * a.qs[1];
    const char *Kp = F & kVarlen ? a.K + (int64_t)kst * a.ks[2] + (int64_t)hk * a.ks[1]
                                 : a.K + (int64_t)b * a.ks[0] + (int64_t)hk * a.ks[1];
    const char *Vp = F & kVarlen ? a.V + (int64_t)kst * a.vs[2] + (int64_t)hk * a.vs[1]
                                 : a.V + (int64_t)b * a.vs[0] + (int64_t)hk * a.vs[1];

    frag qf[KS];

    // ---- DMA staging.  Piece p of a tile = rows RPP*p .. RPP*p+RPP-1 = 1 KiB of LDS; wave w issues pieces
    // w, w+NW, ...  Lane l fills LDS (row = RPP*p + l / CPR, slot = l % CPR) with global chunk slot ^ f(row).
    const int krs = (int)a.ks[2], vrs = (int)a.vs[2];
    // descriptors built from wave-uniform scalars: {base lo, base hi, bytes, flags}; raw buffer (stride 0)
    auto make_rsrc = [&](const char *base, int bytes) {
        const uint64_t ba = (uint64_t)base;
        i32x4 r;
        r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)ba);
        r[1] = __builtin_amdgcn_readfirstlane((int)((uint32_t)(ba >> 32) & 0xffffu));
        r[2] = __builtin_amdgcn_readfirstlane(bytes);
        r[3] = 0x00020000;
        return r;
    };
    // (kVarlen, NK = 0: an empty range -- every load reads 0, and no block is active)
    const i32x4 krsrc = make_rsrc(Kp, F & kVarlen ? (NK > 0 ? (NK - 1) * krs + ROWB : 0) : (N - 1) * krs + ROWB);
    const i32x4 vrsrc = make_rsrc(Vp, F & kVarlen ? (NK > 0 ? (NK - 1) * vrs + ROWB : 0) : (N - 1) * vrs + ROWB);
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds);
    int kvo[PPW], vvo[PPW];
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) {
        const int row = RPP * (wave + pp * NW) + lane / CPR, slot = lane % CPR;
        const int chunk = slot ^ swz<D>(row);
        kvo[pp] = row * krs + chunk * 16;
        vvo[pp] = row * vrs + chunk * 16;
    }
    auto dma_k = [&](int u, int buf) {  // K unit u = keys 64u-32 .. 64u+31 -> LDS K buffer buf
        const int base = (u * 64 - 32) * krs;  // in the VGPR offset: range-checked ("negative" rows wrap -> zero)
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp) dma16(krsrc, lds_base + buf * TILEB + (wave + pp * NW) * 1024, kvo[pp] + base);
    };
    auto dma_v = [&](int t, int buf) {
        const int base = t * 64 * vrs;
#pragma unroll
        for (int pp = 0; pp < PPW; ++pp)
            dma16(vrsrc, lds_base + VBASE + buf * TILEB + (wave + pp * NW) * 1024, vvo[pp] + base);
    };

    int kend = 0, nt = 0, nblk = 0, nb = 0;  // set per pass

    // ---- per-lane swizzled read offsets
    int k_off[KS];  // K row read: row (half*32 + i), chunk 2ks + h
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) k_off[ks] = lds_off<D>(i, 2 * ks + h);
    int v_off[2][DB];  // V transposed read (see fa2_mfma16.hip): u = keys +0..3 / +8..11 of the 16-key step
    {
        const int w = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int db = 0; db < DB; ++db)
                v_off[u][db] = VBASE + lds_off<D>(8 * u + 4 * h + qq, 4 * db + 2 * w + (pp >> 1)) + 8 * (pp & 1);
    }

    f32x16 o[DB];
    float m = -INFINITY, lsum = 0.0f;
    const float c = a.c_log2e;
    // Rescale threshold in log2 units: P may reach 2^kThr before the running max is raised.  bf16 P has the
    // fp32 exponent range (24 leaves 2^24 * N far below fp32 overflow in l and O); f16 P must stay below 65504.
    // On N(0,1) inputs at scale 1 (score sigma ~ 16 log2 units) a threshold of 8 still fired ~20 times per wave
    // and 4096 keys -- each time the whole workgroup waits at the next barrier -- 24 makes it rare.
    constexpr float kThr = sizeof(T) == 2 && __is_same(T, _Float16) ? 12.0f : 60.0f;  // bf16: 60 (round 2): see fa2_a64.hip

    auto qk = [&](f32x16 &s, int koff) {  // koff = buffer base + half * 32 rows
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4 kf = *(LDS_PTR(u32x4))(lds + koff + k_off[ks]);
            s = M::mfma(__builtin_bit_cast(frag, kf), qf[ks], s);
        }
    };
    auto partial = [&](f32x16 &s, int j, float &coeff, bool masked) -> bool {
        if (masked) {
            if constexpr (F & kWindow) {
                const int lim = qrow + wr < NK - 1 ? qrow + wr : NK - 1;
                const int klim = lim - (j * 32 + 4 * h), klo = qrow - wl - (j * 32 + 4 * h);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) > klim || (r & 3) + 8 * (r >> 2) < klo) s[r] = -INFINITY;
            } else {
                int lim = N - 1;
                if (CAUSAL) lim = qrow < lim ? qrow : lim;
                const int klim = lim - (j * 32 + 4 * h);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) > klim) s[r] = -INFINITY;
            }
        }
        float mx = fmaxf(s[0], s[1]);
#pragma unroll
        for (int r = 2; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = half_swap_max(mx) * c;
        const bool fire = !__all(mx - m <= kThr);  // deferred running max, see fa2_mfma16p.hip
        coeff = 1.0f;
        if (fire) {
            const float m_new = fmaxf(m, mx);
            coeff = __builtin_amdgcn_exp2f(m - m_new);
            m = m_new;
        }
        return fire;
    };
    auto finish = [&](f32x16 &s, frag (&pf)[2]) {
        float rs = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -m));
            rs += p;
            pf[r >> 3][r & 7] = (T)p;
        }
        lsum += rs;
    };
    auto rescale = [&](bool fire, float coeff) {
        if (fire) {
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float x = o[db][r];
                    asm volatile("v_mul_f32 %0, %0, %1" : "+v"(x) : "v"(coeff));
                    o[db][r] = x;
                }
            asm volatile("s_nop 7" ::: "memory");
            lsum *= coeff;
        }
    };
    auto pv = [&](frag (&pf)[2], int voff) {  // voff = buffer base + half * 32 rows
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const int rowb = voff + ss * 16 * ROWB;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + rowb + v_off[0][db]));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + rowb + v_off[1][db]));
                const s16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o[db] = M::mfma(__builtin_bit_cast(frag, vf), pf[ss], o[db]);
            }
    };
    auto block_masked = [&](int j) {
        if constexpr (F & kWindow) return (j * 32 + 32 > NK) || (j * 32 < q0 + 31 - wl) || (j * 32 + 31 > q0 + wr);
        else return (CAUSAL && (j * 32 + 31 > q0)) || (j * 32 + 32 > N);
    };

    for (int pass = 0; pass < npass; ++pass) {
        const int qi = pass == 0 ? qi_first : qi_second;
        q0 = qi * BR + wave * 32;
        qrow = q0 + i;
        {
            const int row = qrow < NQ ? qrow : NQ - 1;
            const char *qp = Qp + (int64_t)row * a.qs[2] + h * 16;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) qf[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(qp + ks * 32));
        }
        if constexpr (F & kWindow) {
            // window: the keys of the tile's rows [qi BR - wl, qi BR + BR - 1 + wr]; the loop starts at the 64-key unit t0 of the
            // first one.  Per wave: blocks [jlo, nb) meet its band, the others are skipped
            kend = qi * BR + BR + wr < NK ? qi * BR + BR + wr : NK;
            const int t0 = qi * BR - wl > 0 ? (qi * BR - wl) >> 6 : 0;
            const int jlo = q0 - wl > 0 ? (q0 - wl) >> 5 : 0;
            nt = (kend + 63) >> 6;    // V tiles (loop iterations t0 .. nt-1)
            nblk = (kend + 31) >> 5;  // 32-key blocks of this tile
            {
                const int hi = q0 + 31 + wr < NK - 1 ? q0 + 31 + wr : NK - 1;
                nb = (hi >> 5) + 1 < nblk ? (hi >> 5) + 1 : nblk;
            }
            auto act = [&](int j) { return j >= jlo && j < nb; };
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
            // a row may meet whole blocks before its band starts: a finite floor keeps exp2(m_old - m_new) and exp2(-inf - m) at 0
            // there instead of exp2(-inf + inf); the row's first visible key raises m above it at once (fire below)
            m = -1e30f;
            lsum = 0.0f;

            // ---- prologue: K units t0, t0 + 1 and V tile t0 (the buffers alternate from t0 on)
            dma_k(t0, 0);
            dma_v(t0, 0);
            dma_k(t0 + 1, 1);
            dma_wait();
            __syncthreads();

            f32x16 sA, sB;
            float coeffA = 1.0f, coeffB = 1.0f;
            bool fireA = false, fireB = false;
            frag pf[2];
            if (act(2 * t0)) {
                qk(sA, 32 * ROWB);  // block 2 t0 = rows 32..63 of K unit t0
                fireA = partial(sA, 2 * t0, coeffA, block_masked(2 * t0));
            }
            __syncthreads();    // K unit t0 is overwritten by unit t0 + 2 in iteration t0

            // steady iterations t: block 2t computed, blocks 2t+1 and 2t+2 inside the band for all 32 rows of the wave
            const int ulo = q0 + 31 - wl > 0 ? (q0 + 31 - wl + 31) >> 5 : 0;  // first block without a left-edge mask
            int umax = q0 + wr - 31 < 0 ? -1 : (q0 + wr - 31) >> 5;            // last block without a right-edge mask
            umax = (NK >> 5) - 1 < umax ? (NK >> 5) - 1 : umax;
            int t_head = (jlo + 1) >> 1 > (ulo >> 1) ? (jlo + 1) >> 1 : ulo >> 1;
            t_head = t_head < t0 ? t0 : (t_head > nt ? nt : t_head);
            int t_steady = umax >= 2 ? (umax - 2) / 2 + 1 : 0;
            t_steady = t_steady < t_head ? t_head : (t_steady > nt ? nt : t_steady);

            // head and tail iterations: every block guarded, edge blocks masked
            auto guarded_step = [&](int t) __attribute__((always_inline)) {
                const bool more = t + 1 < nt;
                if (more) {
                    dma_k(t + 2, (t - t0) & 1);
                    dma_v(t + 1, (t + 1 - t0) & 1);
                }
                const int kcur = ((t + 1 - t0) & 1) * TILEB;
                const int vcur = ((t - t0) & 1) * TILEB;
                const int jA = 2 * t, jB = 2 * t + 1, jA2 = 2 * t + 2;
                if (act(jA)) rescale(fireA, coeffA);
                if (act(jB)) qk(sB, kcur);
                if (act(jA)) {
                    finish(sA, pf);
                    pv(pf, vcur);
                }
                if (act(jB)) {
                    fireB = partial(sB, jB, coeffB, block_masked(jB));
                    rescale(fireB, coeffB);
                }
                if (act(jA2)) qk(sA, kcur + 32 * ROWB);
                if (act(jB)) {
                    finish(sB, pf);
                    pv(pf, vcur + 32 * ROWB);
                }
                if (act(jA2)) fireA = partial(sA, jA2, coeffA, block_masked(jA2));
                dma_wait();
                __syncthreads();
            };

            int t = t0;
            for (; t < t_head; ++t) guarded_step(t);
            for (; t < t_steady; ++t) {
                dma_k(t + 2, (t - t0) & 1);
                dma_v(t + 1, (t + 1 - t0) & 1);
                const int kcur = ((t + 1 - t0) & 1) * TILEB;  // K unit t+1: rows 0..31 = block 2t+1, rows 32..63 = block 2t+2
                const int vcur = ((t - t0) & 1) * TILEB;      // V tile t:   rows 0..31 = block 2t,   rows 32..63 = block 2t+1
                rescale(fireA, coeffA);
                qk(sB, kcur);
                finish(sA, pf);
                pv(pf, vcur);
                fireB = partial(sB, 2 * t + 1, coeffB, false);
                rescale(fireB, coeffB);
                qk(sA, kcur + 32 * ROWB);
                finish(sB, pf);
                pv(pf, vcur + 32 * ROWB);
                fireA = partial(sA, 2 * t + 2, coeffA, false);
                dma_wait();
                __syncthreads();
            }
            for (; t < nt; ++t) guarded_step(t);

        } else {
            kend = CAUSAL ? ((qi * BR + BR) < N ? (qi * BR + BR) : N) : N;
            nt = (kend + 63) >> 6;    // V tiles (= loop iterations)
            nblk = (kend + 31) >> 5;  // 32-key blocks of this tile
            nb = nblk;                // ... of this wave (causal: up to its diagonal block)
            if (CAUSAL) nb = (q0 >> 5) + 1 < nblk ? (q0 >> 5) + 1 : nblk;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
            m = -INFINITY;
            lsum = 0.0f;

            // ---- prologue: K units 0, 1 and V tile 0
            dma_k(0, 0);
            dma_v(0, 0);
            dma_k(1, 1);
            dma_wait();
            __syncthreads();

            f32x16 sA, sB;
            float coeffA = 1.0f, coeffB = 1.0f;
            bool fireA = false, fireB = false;
            frag pf[2];
            qk(sA, 32 * ROWB);  // block 0 = rows 32..63 of K unit 0
            fireA = partial(sA, 0, coeffA, block_masked(0));
            __syncthreads();    // K unit 0 is overwritten by unit 2 in iteration 0

            int jm = nb;
            if (CAUSAL) jm = (q0 >> 5) < jm ? (q0 >> 5) : jm;
            if ((N >> 5) < jm) jm = N >> 5;
            int t_steady = (jm - 1) / 2;
            t_steady = t_steady < 0 ? 0 : (t_steady > nt ? nt : t_steady);

            int t = 0;
            for (; t < t_steady; ++t) {
                // both target buffers were released by the barrier that ended iteration t-1; the DMA has the whole
                // iteration to land and is published by the barrier at its end
                dma_k(t + 2, t & 1);
                dma_v(t + 1, (t + 1) & 1);
                const int kcur = ((t + 1) & 1) * TILEB;  // K unit t+1: rows 0..31 = block 2t+1, rows 32..63 = block 2t+2
                const int vcur = (t & 1) * TILEB;        // V tile t:   rows 0..31 = block 2t,   rows 32..63 = block 2t+1
                rescale(fireA, coeffA);
                qk(sB, kcur);
                finish(sA, pf);
                pv(pf, vcur);
                fireB = partial(sB, 2 * t + 1, coeffB, false);
                rescale(fireB, coeffB);
                qk(sA, kcur + 32 * ROWB);
                finish(sB, pf);
                pv(pf, vcur + 32 * ROWB);
                fireA = partial(sA, 2 * t + 2, coeffA, false);
                dma_wait();  // this wave's pieces of (K unit t+2, V tile t+1) have landed; the barrier publishes them
                __syncthreads();
            }
            for (; t < nt; ++t) {
                const bool more = t + 1 < nt;
                if (more) {
                    dma_k(t + 2, t & 1);
                    dma_v(t + 1, (t + 1) & 1);
                }
                const int kcur = ((t + 1) & 1) * TILEB;
                const int vcur = (t & 1) * TILEB;
                const int jA = 2 * t, jB = 2 * t + 1, jA2 = 2 * t + 2;
                if (jA < nb) rescale(fireA, coeffA);
                if (jB < nb) qk(sB, kcur);
                if (jA < nb) {
                    finish(sA, pf);
                    pv(pf, vcur);
                }
                if (jB < nb) {
                    fireB = partial(sB, jB, coeffB, block_masked(jB));
                    rescale(fireB, coeffB);
                }
                if (jA2 < nb) qk(sA, kcur + 32 * ROWB);
                if (jB < nb) {
                    finish(sB, pf);
                    pv(pf, vcur + 32 * ROWB);
                }
                if (jA2 < nb) fireA = partial(sA, jA2, coeffA, block_masked(jA2));
                dma_wait();
                __syncthreads();
            }
        }

        // ---- epilogue (kernels.py:105-108).  A lane owns one ROW of O (columns 32db + 8g + 4h ..+3): stored straight
        // from the accumulators that is 16 eight-byte stores per lane, each instruction touching 32 rows.  Instead the
        // wave's 32 x D tile goes through its own 32*ROWB-byte slice of the (now idle) K/V buffers and leaves as
        // whole rows: ROWB/16 lanes x 16 bytes per row, 1 KiB contiguous per store instruction.
        const float l = half_swap_sum(lsum);
        const float inv = F & kVarlen ? (l > 0.0f ? 1.0f / l : 0.0f) : 1.0f / l;  // kVarlen, a row without a visible key: O = 0
        {
            const int ebase = wave * 32 * ROWB;  // NW * 32 * ROWB <= 4 * TILEB
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    typedef __attribute__((ext_vector_type(4))) T Tx4;
                    Tx4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (T)(o[db][4 * g + j] * inv);
                    *(LDS_PTR(u32x2))(lds + ebase + lds_off<D>(i, 4 * db + g) + 8 * h) = __builtin_bit_cast(u32x2, v);
                }
            // same wave wrote and reads: LDS executes a wave's accesses in order; no other wave touches this slice
            // until the barrier below
            constexpr int RPI = 64 / CPR;  // rows per store instruction (4 at d = 128, 8 at d = 64)
            const int er = lane / CPR, ec = lane % CPR;
            char *ob = F & kVarlen ? a.O + (int64_t)qst * a.os[2] + (int64_t)hh * a.os[1]
                                   : a.O + (int64_t)b * a.os[0] + (int64_t)hh * a.os[1];
#pragma unroll
            for (int k = 0; k < 32 / RPI; ++k) {
                const int r = k * RPI + er;
                const u32x4 val = *(LDS_PTR(u32x4))(lds + ebase + lds_off<D>(r, ec));
                if (q0 + r < NQ) *(u32x4 *)(ob + (int64_t)(q0 + r) * a.os[2] + ec * 16) = val;
            }
        }
        if (qrow < NQ && h == 0) {
            if constexpr (F & kVarlen) {
                T *lp = (T *)a.L + hh * a.ls[1] + qst + qrow;
                *lp = l > 0.0f ? (T)(m + __builtin_amdgcn_logf(l)) : (T)INFINITY;  // no visible key: L = +inf
            } else {
                T *lp = (T *)a.L + b * a.ls[0] + hh * a.ls[1] + qrow;
                *lp = (T)(m + __builtin_amdgcn_logf(l));
            }
        }
        if (pass + 1 < npass) __syncthreads();  // the next pass's DMA reuses the slices
    }  // pass
}

template <typename T, int D, int NW, int F> int launch_t(const Fa2Problem &p, const DmaArgs &a) {
    constexpr int BR = NW * 32;
    const int nq = ((F & kVarlen ? p.max_q : p.N) + BR - 1) / BR;
    const long long nblk = (long long)(p.causal ? (nq + 1) / 2 : nq) * p.B * p.H;  // causal: one workgroup per tile pair
    if (nblk > 0x7fffffffLL) {
        fa2_set_error("mfma16d: grid too large");
        return FA2_ERR_BAD_ARG;
    }
    const dim3 grid((unsigned)nblk), block(NW * 64);
    constexpr size_t smem = 4 * 64 * D * 2;  // 64 KiB (d = 128) / 32 KiB (d = 64)
    if constexpr (F & kWindow) {  // (p.causal is 0: the causal mask is in wr, or in the band)
        hipLaunchKernelGGL((fa2_fwd_mfma16d_kernel<T, D, NW, false, F>), grid, block, smem, p.stream, a);
    } else {
        if (p.causal)
            hipLaunchKernelGGL((fa2_fwd_mfma16d_kernel<T, D, NW, true>), grid, block, smem, p.stream, a);
        else
            hipLaunchKernelGGL((fa2_fwd_mfma16d_kernel<T, D, NW, false>), grid, block, smem, p.stream, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("mfma16d kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <typename T, int F> int launch_d(const Fa2Problem &p, const DmaArgs &a, int waves) {
    if (p.d == 128) return waves == 8 ? launch_t<T, 128, 8, F>(p, a) : launch_t<T, 128, 4, F>(p, a);
    return waves == 8 ? launch_t<T, 64, 8, F>(p, a) : launch_t<T, 64, 4, F>(p, a);
}

// the f16 kernels of form F: defined and instantiated in fa2_mfma16d_f16.hip
template <int F> int launch_f16(const Fa2Problem &p, const DmaArgs &a, int waves);

}  // namespace fa2_mfma16d
