// fa2_mfma16dv.hip -- the packed (varlen, GQA) f16 / bf16 forward at d = 192, d_v = 128 (variant "mfma16dv", fa2_fwd_varlen_dv):
// un-absorbed MLA prefill, where a head's query and key are 128 "nope" columns followed by 64 rotary ones and its value is 128 wide.
//
// It is the varlen GQA form of fa2_mfma16d_kernel.h (F = kWindow | kVarlen | kGqa) written out for this one shape: 4 waves x 32 query rows per
// workgroup, one tile per workgroup and sequence, the 64-key K unit / V tile ring filled by LDS-DMA, QK^T of block j + 1 under the
// softmax of block j, the band of fa2_varlen_seq / fa2_varlen_band with blocks outside a wave's band skipped and blocks across its
// edges masked, a row without a visible key O = 0 and L = +inf.  (The form it starts from runs the causal mask as a band and has no
// tile pairs; neither has this one.)  The arithmetic is that kernel's, statement for statement; P.V is its d = 128 code.
//
// What is new is the K image.  LDS-DMA writes lane-linearly, so rows cannot be padded, and a 384-byte row is 1.5 bank rows: neither
// swz<128> nor swz<64> (fa2_mfma.h) is conflict-free on it.  A K unit is therefore staged as TWO images, each in a layout the
// d = 128 / d = 64 kernels already read without conflicts:
//   image A: columns   0..127, 64 rows of 256 bytes (swz<128>), 16 one-KiB pieces of 4 rows
//   image B: columns 128..191, 64 rows of 128 bytes (swz< 64>),  8 one-KiB pieces of 8 rows
// and the k-loop of QK^T crosses them: k-steps 0..7 read image A, k-steps 8..11 image B, against 12 resident Q fragments.
// LDS: 2 K units x (16 + 8) KiB | 2 V tiles x 16 KiB = 80 KiB, half of the CU's 160 KiB; the epilogue's O tile goes through the
// (then idle) V tiles.
#include "fa2_common.h"
#include "fa2_mfma.h"

namespace {

constexpr int kD = 192, kDV = 128;
constexpr int kNW = 4, kBR = kNW * 32;
constexpr int kRowA = 256, kRowB = 128, kRowV = 256;     // bytes per LDS row of image A, image B, a V tile
constexpr int kImgA = 64 * kRowA, kImgB = 64 * kRowB;    // 16 KiB, 8 KiB
constexpr int kUnit = kImgA + kImgB, kTileV = 64 * kRowV;  // a K unit (24 KiB), a V tile (16 KiB)
constexpr int kVBase = 2 * kUnit;                        // LDS: Kunit0 (A | B) | Kunit1 (A | B) | Vtile0 | Vtile1
constexpr int kSmem = 2 * kUnit + 2 * kTileV;            // 80 KiB
constexpr int kPA = kImgA / 1024 / kNW, kPB = kImgB / 1024 / kNW, kPV = kTileV / 1024 / kNW;  // DMA pieces per wave: 4, 2, 4
constexpr int kKS = kD / 16, kKSA = 8;                   // 12 k-steps, the first 8 in image A
constexpr int kDB = kDV / 32;                            // 32-column blocks of O

struct DvArgs {
    const char *Q, *K, *V;
    char *O, *L;
    int64_t qs[3], ks[3], vs[3], os[3];  // -, head, token strides in bytes
    int64_t ls[2];
    int B, H;
    float c_log2e;
    int wl, wr;  // raw window sides (-1 = unbounded), shifted per sequence by fa2_varlen_band
    int causal;
    const int32_t *cu_q, *cu_k;
    int max_q, max_k, total_q, total_k;
    int gqa;  // query heads per KV head
};

template <typename T>
__global__ __launch_bounds__(kNW * 64, 2) void fa2_fwd_mfma16dv_kernel(const DvArgs a) {
    using M = Mma<T>;
    using frag = typename M::frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS_PTR(char) lds = (LDS_PTR(char))smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (M0, scalar branches)
    const int i = lane & 31, h = lane >> 5;

    const int nq = (a.max_q + kBR - 1) / kBR, nbh = a.B * a.H;  // one tile per workgroup
    int bh, qi;
    {
        const int bid = blockIdx.x;
        if ((nbh & 7) == 0) {  // whole (b, h) per XCD (speed only)
            const int slot = bid >> 3, batch = slot / nq;
            bh = batch * 8 + (bid & 7);
            qi = slot - batch * nq;
        } else {
            bh = bid / nq;
            qi = bid % nq;
        }
    }
    const int b = bh / a.H, hh = bh - b * a.H;

    int qst, NQ, kst, NK;
    fa2_varlen_seq(a.cu_q, b, a.total_q, a.max_q, qst, NQ);
    fa2_varlen_seq(a.cu_k, b, a.total_k, a.max_k, kst, NK);
    qst = __builtin_amdgcn_readfirstlane(qst);
    NQ = __builtin_amdgcn_readfirstlane(NQ);
    kst = __builtin_amdgcn_readfirstlane(kst);
    NK = __builtin_amdgcn_readfirstlane(NK);
    if (qi * kBR >= NQ) return;  // (whole workgroup, before any barrier)
    int wl, wr;
    fa2_varlen_band(NQ, NK, a.causal, a.wl, a.wr, wl, wr);
    const int hk = hh / a.gqa;
    const char *Qp = a.Q + (int64_t)qst * a.qs[2] + (int64_t)hh * a.qs[1];
    const char *Kp = a.K + (int64_t)kst * a.ks[2] + (int64_t)hk * a.ks[1];
    const char *Vp = a.V + (int64_t)kst * a.vs[2] + (int64_t)hk * a.vs[1];

    const int q0 = qi * kBR + wave * 32, qrow = q0 + i;

    // ---- Q: 12 resident fragments (k-step ks = columns 16 ks .. 16 ks + 15, this lane's half h of it)
    frag qf[kKS];
    {
        const int row = qrow < NQ ? qrow : NQ - 1;
        const char *qp = Qp + (int64_t)row * a.qs[2] + h * 16;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) qf[ks] = __builtin_bit_cast(frag, *(const u32x4 *)(qp + ks * 32));
    }

    // ---- DMA staging.  A piece is 1 KiB of LDS; wave w issues pieces w, w + 4, ... of each image.  Lane l fills (row, slot) of its
    // piece with the global chunk slot ^ swz(row) of that row: image A takes chunks 0..15 of a K row, image B chunks 16..23.
    const int krs = (int)a.ks[2], vrs = (int)a.vs[2];
    auto make_rsrc = [&](const char *base, int bytes) {  // raw buffer (stride 0) from wave-uniform scalars
        const uint64_t ba = (uint64_t)base;
        i32x4 r;
        r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)ba);
        r[1] = __builtin_amdgcn_readfirstlane((int)((uint32_t)(ba >> 32) & 0xffffu));
        r[2] = __builtin_amdgcn_readfirstlane(bytes);
        r[3] = 0x00020000;
        return r;
    };
    // rows past NK and the "negative" rows of K unit 0 fall outside the range and read 0 (NK = 0: an empty range)
    const i32x4 krsrc = make_rsrc(Kp, NK > 0 ? (NK - 1) * krs + kD * 2 : 0);
    const i32x4 vrsrc = make_rsrc(Vp, NK > 0 ? (NK - 1) * vrs + kDV * 2 : 0);
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds);
    int kao[kPA], kbo[kPB], vvo[kPV];
#pragma unroll
    for (int pp = 0; pp < kPA; ++pp) {
        const int row = 4 * (wave + pp * kNW) + lane / 16, slot = lane % 16;
        kao[pp] = row * krs + (slot ^ swz<128>(row)) * 16;
    }
#pragma unroll
    for (int pp = 0; pp < kPB; ++pp) {
        const int row = 8 * (wave + pp * kNW) + lane / 8, slot = lane % 8;
        kbo[pp] = row * krs + kRowA + (slot ^ swz<64>(row)) * 16;
    }
#pragma unroll
    for (int pp = 0; pp < kPV; ++pp) {
        const int row = 4 * (wave + pp * kNW) + lane / 16, slot = lane % 16;
        vvo[pp] = row * vrs + (slot ^ swz<128>(row)) * 16;
    }
    auto dma_k = [&](int u, int buf) {  // K unit u = keys 64u-32 .. 64u+31 -> LDS K buffer buf
        const int base = (u * 64 - 32) * krs;  // in the VGPR offset: range-checked ("negative" rows wrap -> zero)
#pragma unroll
        for (int pp = 0; pp < kPA; ++pp) dma16(krsrc, lds_base + buf * kUnit + (wave + pp * kNW) * 1024, kao[pp] + base);
#pragma unroll
        for (int pp = 0; pp < kPB; ++pp) dma16(krsrc, lds_base + buf * kUnit + kImgA + (wave + pp * kNW) * 1024, kbo[pp] + base);
    };
    auto dma_v = [&](int t, int buf) {
        const int base = t * 64 * vrs;
#pragma unroll
        for (int pp = 0; pp < kPV; ++pp) dma16(vrsrc, lds_base + kVBase + buf * kTileV + (wave + pp * kNW) * 1024, vvo[pp] + base);
    };

    // ---- per-lane swizzled read offsets
    int k_off[kKS];  // K row read: row i of a 32-row half, chunk 2 ks + h of image A (ks < 8) or 2 (ks - 8) + h of image B
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks)
        k_off[ks] = ks < kKSA ? lds_off<128>(i, 2 * ks + h) : kImgA + lds_off<64>(i, 2 * (ks - kKSA) + h);
    int v_off[2][kDB];  // V transposed read (see fa2_mfma16.hip): u = keys +0..3 / +8..11 of the 16-key step
    {
        const int w = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int db = 0; db < kDB; ++db)
                v_off[u][db] = kVBase + lds_off<128>(8 * u + 4 * h + qq, 4 * db + 2 * w + (pp >> 1)) + 8 * (pp & 1);
    }

    f32x16 o[kDB];
    float m, lsum;
    const float c = a.c_log2e;
    // Rescale threshold in log2 units (fa2_mfma16d.hip): bf16 P has the fp32 exponent range, f16 P must stay below 65504.
    constexpr float kThr = __is_same(T, _Float16) ? 12.0f : 60.0f;

    auto qk = [&](f32x16 &s, int kbuf, int half) {  // kbuf = byte offset of the K unit, half = rows 32 half .. 32 half + 31
        const int offA = kbuf + half * 32 * kRowA, offB = kbuf + half * 32 * kRowB;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) {
            const u32x4 kf = *(LDS_PTR(u32x4))(lds + (ks < kKSA ? offA : offB) + k_off[ks]);
            s = M::mfma(__builtin_bit_cast(frag, kf), qf[ks], s);
        }
    };
    auto partial = [&](f32x16 &s, int j, float &coeff, bool masked) -> bool {
        if (masked) {
            const int lim = qrow + wr < NK - 1 ? qrow + wr : NK - 1;
            const int klim = lim - (j * 32 + 4 * h), klo = qrow - wl - (j * 32 + 4 * h);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((r & 3) + 8 * (r >> 2) > klim || (r & 3) + 8 * (r >> 2) < klo) s[r] = -INFINITY;
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
            for (int db = 0; db < kDB; ++db)
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
    auto pv = [&](frag (&pf)[2], int voff) {  // voff = V tile offset + half * 32 rows
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
            for (int db = 0; db < kDB; ++db) {
                const int rowb = voff + ss * 16 * kRowV;
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + rowb + v_off[0][db]));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_PTR(s16x4))(lds + rowb + v_off[1][db]));
                const s16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o[db] = M::mfma(__builtin_bit_cast(frag, vf), pf[ss], o[db]);
            }
    };
    auto block_masked = [&](int j) { return (j * 32 + 32 > NK) || (j * 32 < q0 + 31 - wl) || (j * 32 + 31 > q0 + wr); };

    // ---- the key loop of fa2_mfma16d.hip's windowed form: the keys of the tile's rows [qi BR - wl, qi BR + BR - 1 + wr], from the
    // 64-key unit t0 of the first one.  Per wave: blocks [jlo, nb) meet its band, the others are skipped
    const int kend = qi * kBR + kBR + wr < NK ? qi * kBR + kBR + wr : NK;
    const int t0 = qi * kBR - wl > 0 ? (qi * kBR - wl) >> 6 : 0;
    const int jlo = q0 - wl > 0 ? (q0 - wl) >> 5 : 0;
    const int nt = (kend + 63) >> 6;    // V tiles (loop iterations t0 .. nt-1)
    const int nblk = (kend + 31) >> 5;  // 32-key blocks of this tile
    int nb;
    {
        const int hi = q0 + 31 + wr < NK - 1 ? q0 + 31 + wr : NK - 1;
        nb = (hi >> 5) + 1 < nblk ? (hi >> 5) + 1 : nblk;
    }
    auto act = [&](int j) { return j >= jlo && j < nb; };
#pragma unroll
    for (int db = 0; db < kDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
    // a row may meet whole blocks before its band starts: a finite floor keeps exp2(m_old - m_new) and exp2(-inf - m) at 0 there
    // instead of exp2(-inf + inf); the row's first visible key raises m above it at once (fire)
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
        qk(sA, 0, 1);  // block 2 t0 = rows 32..63 of K unit t0
        fireA = partial(sA, 2 * t0, coeffA, block_masked(2 * t0));
    }
    __syncthreads();  // K unit t0 is overwritten by unit t0 + 2 in iteration t0

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
        const int kcur = ((t + 1 - t0) & 1) * kUnit;
        const int vcur = ((t - t0) & 1) * kTileV;
        const int jA = 2 * t, jB = 2 * t + 1, jA2 = 2 * t + 2;
        if (act(jA)) rescale(fireA, coeffA);
        if (act(jB)) qk(sB, kcur, 0);
        if (act(jA)) {
            finish(sA, pf);
            pv(pf, vcur);
        }
        if (act(jB)) {
            fireB = partial(sB, jB, coeffB, block_masked(jB));
            rescale(fireB, coeffB);
        }
        if (act(jA2)) qk(sA, kcur, 1);
        if (act(jB)) {
            finish(sB, pf);
            pv(pf, vcur + 32 * kRowV);
        }
        if (act(jA2)) fireA = partial(sA, jA2, coeffA, block_masked(jA2));
        dma_wait();
        __syncthreads();
    };

    int t = t0;
    for (; t < t_head; ++t) guarded_step(t);
    for (; t < t_steady; ++t) {
        // both target buffers were released by the barrier that ended iteration t-1; the DMA has the whole iteration to land and
        // is published by the barrier at its end
        dma_k(t + 2, (t - t0) & 1);
        dma_v(t + 1, (t + 1 - t0) & 1);
        const int kcur = ((t + 1 - t0) & 1) * kUnit;   // K unit t+1: rows 0..31 = block 2t+1, rows 32..63 = block 2t+2
        const int vcur = ((t - t0) & 1) * kTileV;      // V tile t:   rows 0..31 = block 2t,   rows 32..63 = block 2t+1
        rescale(fireA, coeffA);
        qk(sB, kcur, 0);
        finish(sA, pf);
        pv(pf, vcur);
        fireB = partial(sB, 2 * t + 1, coeffB, false);
        rescale(fireB, coeffB);
        qk(sA, kcur, 1);
        finish(sB, pf);
        pv(pf, vcur + 32 * kRowV);
        fireA = partial(sA, 2 * t + 2, coeffA, false);
        dma_wait();
        __syncthreads();
    }
    for (; t < nt; ++t) guarded_step(t);

    // ---- epilogue.  The wave's 32 x 128 tile of O goes through its own 8 KiB slice of the (now idle) V tiles and leaves as whole
    // rows: 16 lanes x 16 bytes per row, 1 KiB contiguous per store instruction (fa2_mfma16d.hip at d = 128).
    const float l = half_swap_sum(lsum);
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // a row without a visible key: O = 0
    {
        const int ebase = kVBase + wave * 32 * kRowV;  // 4 x 8 KiB = the two V tiles
#pragma unroll
        for (int db = 0; db < kDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                typedef __attribute__((ext_vector_type(4))) T Tx4;
                Tx4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (T)(o[db][4 * g + j] * inv);
                *(LDS_PTR(u32x2))(lds + ebase + lds_off<128>(i, 4 * db + g) + 8 * h) = __builtin_bit_cast(u32x2, v);
            }
        // same wave wrote and reads: LDS executes a wave's accesses in order; no other wave touches this slice
        const int er = lane / 16, ec = lane % 16;
        char *ob = a.O + (int64_t)qst * a.os[2] + (int64_t)hh * a.os[1];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = k * 4 + er;
            const u32x4 val = *(LDS_PTR(u32x4))(lds + ebase + lds_off<128>(r, ec));
            if (q0 + r < NQ) *(u32x4 *)(ob + (int64_t)(q0 + r) * a.os[2] + ec * 16) = val;
        }
    }
    if (qrow < NQ && h == 0) {
        T *lp = (T *)a.L + hh * a.ls[1] + qst + qrow;
        *lp = l > 0.0f ? (T)(m + __builtin_amdgcn_logf(l)) : (T)INFINITY;  // no visible key: L = +inf
    }
}

template <typename T> int launch_t(const Fa2Problem &p, const DvArgs &a) {
    const int nq = (p.max_q + kBR - 1) / kBR;
    const long long nblk = (long long)nq * p.B * p.H;
    if (nblk > 0x7fffffffLL) {
        fa2_set_error("mfma16dv: grid too large");
        return FA2_ERR_BAD_ARG;
    }
    static Fa2DeviceLatch attr_done;  // more than 64 KiB of dynamic LDS: opt in, once per instantiation and device
    if (attr_done.need()) {
        (void)hipFuncSetAttribute((const void *)fa2_fwd_mfma16dv_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, kSmem);
        attr_done.mark();
    }
    hipLaunchKernelGGL((fa2_fwd_mfma16dv_kernel<T>), dim3((unsigned)nblk), dim3(kNW * 64), kSmem, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("mfma16dv kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// What the kernel takes, the 32-bit buffer offsets judged on one sequence (max_seqlen_k x row stride, with 512 rows of overrun).
bool fa2_mfma16dv_supports(const Fa2Problem &p) {
    if (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16) return false;
    if (p.d != kD || p.dv != kDV) return false;
    if (!(p.scale > 0.0f) || !(p.scale < INFINITY)) return false;
    if (p.qs[3] != 1 || p.ks[3] != 1 || p.vs[3] != 1 || p.os[3] != 1) return false;
    for (int k = 1; k < 3; ++k)  // (head and token strides: 16-byte loads of Q / K / V rows, 16-byte stores of O rows)
        if ((p.qs[k] & 7) || (p.ks[k] & 7) || (p.vs[k] & 7) || (p.os[k] & 7)) return false;
    if (!aligned16(p.Q) || !aligned16(p.K) || !aligned16(p.V) || !aligned16(p.O)) return false;
    // a key row past the sequence must start past the descriptor's range, which ends with the last row: rows do not overlap
    if (p.ks[2] < kD || p.vs[2] < kDV) return false;
    if ((int64_t)(p.max_k + 512) * p.ks[2] * 2 >= (1LL << 31) || (int64_t)(p.max_k + 512) * p.vs[2] * 2 >= (1LL << 31)) return false;
    return true;
}

int fa2_launch_mfma16dv(const Fa2Problem &p, int gqa) {
    if (!fa2_mfma16dv_supports(p)) {
        fa2_set_error("mfma16dv kernel: needs f16/bf16, d = 192 and d_v = 128, unit d-stride, 16-byte aligned rows of Q, K, V and O, "
                      "scale > 0, max_seqlen_k * row stride < 2 GiB (got dtype %d, d=%d, d_v=%d)", p.dtype, p.d, p.dv);
        return FA2_ERR_UNSUPPORTED;
    }
    DvArgs a;
    a.Q = (const char *)p.Q; a.K = (const char *)p.K; a.V = (const char *)p.V;
    a.O = (char *)p.O; a.L = (char *)p.L;
    for (int k = 0; k < 3; ++k) {
        a.qs[k] = p.qs[k] * 2; a.ks[k] = p.ks[k] * 2; a.vs[k] = p.vs[k] * 2; a.os[k] = p.os[k] * 2;
    }
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.B = p.B; a.H = p.H;
    a.c_log2e = (float)((double)p.scale * FA2_LOG2E);
    a.wl = p.wl; a.wr = p.wr; a.causal = p.causal;
    a.cu_q = p.cu_q; a.cu_k = p.cu_k; a.max_q = p.max_q; a.max_k = p.max_k; a.total_q = p.total_q; a.total_k = p.total_k;
    a.gqa = gqa;
    if (p.max_q == 0) return FA2_OK;  // no query rows anywhere
    return p.dtype == FA2_DTYPE_BF16 ? launch_t<__bf16>(p, a) : launch_t<_Float16>(p, a);
}
