// fa2_indexer_prep.hip -- the MLA indexer's FRONT END (include/fa2_fwd.h): fa2_mla_indexer_prepare_q / _varlen turn index queries into
// the operands the score kernels read (rotary, the 128-point Hadamard transform, the power-of-two row quantisation, the row scale
// folded into the weights), fa2_mla_indexer_append_rot / _varlen_rot do the same to new index keys and store them in the cache.  One
// launch each, in place of the dozen torch launches of the model's own code.
//
// Work layout.  A row has 128 columns.  SIXTEEN LANES own a row, lane s of them its columns 8 s .. 8 s + 7 -- one 16-byte load -- so a
// wave holds four rows and a block of four waves (dim3(64, 4)) sixteen.  Everything a row needs from its other columns crosses lanes
// INSIDE those sixteen, which are one DPP row: no LDS, no barrier, nothing between waves.
//   rotary     interleaved pairs (2i, 2i + 1) sit in the lane.  The half pairing (i, i + rotary_dim / 2) with rotary_dim 16, 32, 64 or
//              128 pairs lane s with s ^ 1, 2, 4 or 8: the four packed words of the partner come by the exchange below, the table
//              columns by one 16-byte load (8 bytes interleaved).  Any other even rotary_dim, or tables whose rows are not 16-byte
//              aligned, take the element path: the partner column is read from the source row again (an L1 hit), the tables one
//              element at a time.  The same bits either way (rot_pair, one rounding to the dtype).
//   Hadamard   strides 1, 2, 4 are butterflies between the lane's own registers, strides 8, 16, 32, 64 between lane s and s ^ 1, 2, 4,
//              8: the lower lane keeps a + b, the upper a - b with a the lower lane's value.  Every stage is a set of independent fp32
//              additions, so the order the pairs are visited in does not matter and the result is the torch restatement's
//              (hadamard_rotate) bit for bit.  Then one multiplication by (float)2^-3.5 and one rounding to the dtype.
//   exchange   s ^ 1, s ^ 2: DPP quad_perm; s ^ 8: DPP row_ror:8; s ^ 4: ds_swizzle in bit mode (gfx950 has no DPP control that
//              reaches it).  Every lane of a wave runs every exchange: a group without a row carries zeros, nothing returns early.
//   amax       |h| over the lane's eight columns, then fmaxf across the same four exchanges.
//   stores     fp8: the lane's eight bytes as one uint2; 16 bits: one uint4; lane 0 of the group writes the row's scale (keys) or
//              weights_out (queries).  Ordinary vector stores.
// The matrix cores are not used: an MFMA against a +-1 matrix sums 128 products in the hardware's order, not in the butterfly's, and
// the operation moves 384 bytes a row -- it is bound by memory, not by arithmetic.
//
// Query form: blockIdx.x is the token (b, qi) or the packed row, blockIdx.y a tile of sixteen heads, heads fastest -- the rows of a
// block share one position, so the table row addresses are scalar.  A last tile with fewer than sixteen heads carries zeros in the
// groups past H_I.  Key form: sixteen consecutive tokens a block; sequences, the clamp, the drop past the capacity, the page lookup
// and the lengths are fa2_decode_append_q.hip's (locate below restates its RPW = 4 form), a position per row.
//
// Arithmetic: fa2_append_arith.h's rot_pair, fp8_scaled and fp8_pack2; the power-of-two scale is fa2_decode_append_q.hip's pow2_scale,
// restated here, so the bytes and scales are mla_indexer_append's on the same h.
#include "fa2_indexer.h"
#include "fa2_decode.h"
#include "fa2_append_arith.h"

namespace {

#pragma clang fp contract(off)

constexpr int kWaves = 4, kRows = 4 * kWaves;  // waves and rows per block

// How a launch reads and writes, decided on the host; uniform over the grid.
struct PrepForm {
    int32_t src_vec;   // source rows 16-byte aligned: one uint4 a lane
    int32_t dst_vec;   // destination rows contiguous and aligned to the lane's store
    int32_t rot_fast;  // the exchange path of the rotation (above)
    int32_t hadamard;
};

// The value of lane s ^ X of the 16-lane row.
template <int X> __device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    static_assert(X == 1 || X == 2 || X == 4 || X == 8, "inside a DPP row");
    if constexpr (X == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);        // quad_perm:[1,0,3,2]
    else if constexpr (X == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);   // quad_perm:[2,3,0,1]
    else if constexpr (X == 4) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);                    // and 0x1f, xor 4
    else return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);                        // row_ror:8
}
template <int X> __device__ __forceinline__ float lane_xor(float v) {
    return __builtin_bit_cast(float, lane_xor<X>(__builtin_bit_cast(uint32_t, v)));
}
template <int X> __device__ __forceinline__ uint4 lane_xor(const uint4 &u) {
    return make_uint4(lane_xor<X>(u.x), lane_xor<X>(u.y), lane_xor<X>(u.z), lane_xor<X>(u.w));
}

// One butterfly stage across lanes: `hi` is bit X of the lane's index in its row.
template <int X> __device__ __forceinline__ void cross_stage(float (&v)[8], bool hi) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float p = lane_xor<X>(v[k]);
        v[k] = hi ? p - v[k] : v[k] + p;
    }
}

// h = H_128 v / sqrt(128) in fp32, before the rounding to the dtype.  s: the lane's index in its row.
__device__ __forceinline__ void hadamard128(float (&v)[8], int s) {
#pragma unroll
    for (int st = 1; st < 8; st <<= 1)
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (!(k & st)) {
                const float a = v[k], b = v[k + st];
                v[k] = a + b;
                v[k + st] = a - b;
            }
    cross_stage<1>(v, s & 1);
    cross_stage<2>(v, s & 2);
    cross_stage<4>(v, s & 4);
    cross_stage<8>(v, s & 8);
    constexpr float c = (float)0.08838834764831845;  // 128 ** -0.5
    // Each product is pinned in its register as an fp32 value: the compiler otherwise folds it into the f16 conversion that follows
    // (v_fma_mixlo_f16), which rounds the exact product ONCE where the statement rounds to fp32 and then to f16 -- an ulp of one
    // element in some 10^4.
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = v[k] * c;
        asm volatile("" : "+v"(v[k]));
    }
}

__device__ __forceinline__ float row16_amax(const float (&v)[8]) {
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(v[k]));
    m = fmaxf(m, lane_xor<1>(m));
    m = fmaxf(m, lane_xor<2>(m));
    m = fmaxf(m, lane_xor<4>(m));
    return fmaxf(m, lane_xor<8>(m));
}

// fa2_decode_append_q.hip's pow2_scale: the smallest power of two with amax / scale <= top, 1 for amax = 0.
template <int KV> __device__ __forceinline__ float pow2_scale(float amax) {
    constexpr float top = KV == FA2_DTYPE_F8E4M3 ? 448.0f : 57344.0f;
    const uint32_t q = __builtin_bit_cast(uint32_t, __fdiv_rn(amax, top));
    if (q == 0) return 1.0f;
    const uint32_t e = (q >> 23) + ((q & 0x7fffffu) ? 1u : 0u);
    return __builtin_bit_cast(float, (e < 254u ? e : 254u) << 23);
}

template <class E> __device__ __forceinline__ void round8(float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = E::widen(E::narrow(v[k]));
}

template <class E> __device__ __forceinline__ uint4 narrow8(const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)E::narrow(v[2 * k]) | ((uint32_t)E::narrow(v[2 * k + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The rotary arguments of a row: its table rows (null: no rotation) and the call's pairing.
struct RowRot {
    const char *cosr, *sinr;
    int rd;
    bool interleaved;
};

// Steps 1 and 2 of a row: v = the lane's eight columns of h, already rounded to the dtype and widened again (what the quantisation
// divides and what a 16-bit destination stores).  live: the group has a row (src is then its column 0).  Called by every lane.
template <class E> __device__ __forceinline__ void transform_row(bool live, const char *src, const RowRot &rr, const PrepForm &f, int s,
                                                                 float (&v)[8]) {
    uint4 xu = make_uint4(0, 0, 0, 0);
    if (live) {
        if (f.src_vec) xu = *(const uint4 *)(src + s * 16);
        else {
            const uint16_t *p = (const uint16_t *)src + s * 8;
            xu = make_uint4(p[0] | (uint32_t)p[1] << 16, p[2] | (uint32_t)p[3] << 16, p[4] | (uint32_t)p[5] << 16, p[6] | (uint32_t)p[7] << 16);
        }
    }
    widen8<E>(xu, v);
    const int rd = rr.rd, half = rd >> 1, col = 8 * s;
    if (rr.cosr && f.rot_fast) {  // (uniform) rd % 16 == 0: a lane's unit is inside the rotary range or outside it
        const bool rot = live && col < rd;
        if (rr.interleaved) {
            if (rot) {
                const uint2 cu = *(const uint2 *)(rr.cosr + col), su = *(const uint2 *)(rr.sinr + col);  // table columns 4 s .. 4 s + 3
                const uint32_t cw[2] = {cu.x, cu.y}, sw[2] = {su.x, su.y};
                float o[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float cc = E::widen((uint16_t)(k & 1 ? cw[k >> 1] >> 16 : cw[k >> 1] & 0xffffu));
                    const float ss = E::widen((uint16_t)(k & 1 ? sw[k >> 1] >> 16 : sw[k >> 1] & 0xffffu));
                    o[2 * k] = rot_pair<float>(v[2 * k], v[2 * k + 1], cc, ss, true);
                    o[2 * k + 1] = rot_pair<float>(v[2 * k + 1], v[2 * k], cc, ss, false);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = o[k];
                round8<E>(v);
            }
        } else {  // the partner unit is half / 8 = 1, 2, 4 or 8 lanes away, by xor
            uint4 yu;
            switch (half >> 3) {  // (uniform)
            case 1: yu = lane_xor<1>(xu); break;
            case 2: yu = lane_xor<2>(xu); break;
            case 4: yu = lane_xor<4>(xu); break;
            default: yu = lane_xor<8>(xu); break;
            }
            if (rot) {
                const bool first = col < half;
                const int ci = first ? col : col - half;
                float y[8], cs[8], sn[8];
                widen8<E>(yu, y);
                widen8<E>(*(const uint4 *)(rr.cosr + ci * 2), cs);
                widen8<E>(*(const uint4 *)(rr.sinr + ci * 2), sn);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = rot_pair<float>(v[k], y[k], cs[k], sn[k], first);
                round8<E>(v);
            }
        }
    } else if (rr.cosr) {  // the element path: any even rd, any alignment
        const uint16_t *sb = (const uint16_t *)src, *cb = (const uint16_t *)rr.cosr, *nb = (const uint16_t *)rr.sinr;
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = col + k;
            o[k] = v[k];
            if (live && c < rd) {
                const bool first = rr.interleaved ? !(k & 1) : c < half;
                const int ci = rr.interleaved ? c >> 1 : (first ? c : c - half);
                const float y = rr.interleaved ? v[k ^ 1] : E::widen(sb[first ? c + half : c - half]);
                o[k] = E::widen(E::narrow(rot_pair<float>(v[k], y, E::widen(cb[ci]), E::widen(nb[ci]), first)));
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = o[k];
    }
    if (f.hadamard) {
        hadamard128(v, s);
        round8<E>(v);
    }
}

// Step 3 and the store of the lane's eight columns.  OUT: the fp8 format, or 0 for the row's own dtype.  dst: byte 0 of the row;
// cds: its column stride in elements (read without dst_vec only).  Returns the row's scale (1 for OUT = 0).  Called by every lane.
template <class E, int OUT> __device__ __forceinline__ float store_row(bool live, const float (&v)[8], char *dst, int64_t cds, const PrepForm &f,
                                                                       int s) {
    if constexpr (OUT == 0) {
        if (live) {
            const uint4 u = narrow8<E>(v);
            if (f.dst_vec) *(uint4 *)(dst + s * 16) = u;
            else {
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) ((uint16_t *)dst)[(int64_t)(8 * s + k) * cds] = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
            }
        }
        return 1.0f;
    } else {
        const float scale = pow2_scale<OUT>(row16_amax(v));
        if (live) {
            float q[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) q[k] = fp8_scaled<OUT>(v[k], scale);
            int lo = fp8_pack2<OUT, false>(q[0], q[1], 0), hi = fp8_pack2<OUT, false>(q[4], q[5], 0);
            lo = fp8_pack2<OUT, true>(q[2], q[3], lo);
            hi = fp8_pack2<OUT, true>(q[6], q[7], hi);
            if (f.dst_vec) *(uint2 *)(dst + s * 8) = make_uint2((uint32_t)lo, (uint32_t)hi);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) ((uint8_t *)dst)[(int64_t)(8 * s + k) * cds] = (uint8_t)((uint32_t)(k < 4 ? lo : hi) >> (8 * (k & 3)));
            }
        }
        return scale;
    }
}

// ---- queries ---------------------------------------------------------------------------------------------------------------------
template <class E, int OUT, bool PK>
__global__ __launch_bounds__(64 * kWaves) void fa2_indexer_prep_q_kernel(const Fa2IndexerPrepProblem a, const PrepForm f) {
    constexpr int64_t osz = OUT == 0 ? 2 : 1;
    const int s = threadIdx.x & 15;
    const int head = blockIdx.y * kRows + threadIdx.y * 4 + (threadIdx.x >> 4);
    const bool live = head < a.H;
    // the token: uniform over the block
    int b, n;
    int64_t t, i, orow;  // the row of the sources' token axis, the query's index in its sequence, the output row of head 0
    if constexpr (PK) {
        int st;
        if (!fa2_varlen_owner(a.cu_q, a.B, a.total_q, a.max_q, (int)blockIdx.x, b, st, n)) return;  // (the whole block)
        t = blockIdx.x;
        i = t - st;
        orow = t * a.H;
    } else {
        b = blockIdx.x / a.N_q;
        n = a.N_q;
        t = i = blockIdx.x % a.N_q;
        orow = (int64_t)b * a.H * a.N_q + i;
    }
    RowRot rr = {nullptr, nullptr, a.rotary_dim, a.interleaved != 0};
    if (a.cos) {
        int64_t pos = (int64_t)a.seqlens[b] - n + i;
        pos = pos < 0 ? 0 : (pos > a.S_rot - 1 ? a.S_rot - 1 : pos);
        rr.cosr = (const char *)a.cos + pos * a.cos_stride * 2;
        rr.sinr = (const char *)a.sin + pos * a.sin_stride * 2;
    }
    const char *src = (const char *)a.Q + ((int64_t)b * a.qs[0] + (int64_t)head * a.qs[1] + t * a.qs[2]) * 2;
    const int64_t row = PK ? orow + head : orow + (int64_t)head * a.N_q;
    float v[8];
    transform_row<E>(live, src, rr, f, s, v);
    const float scale = store_row<E, OUT>(live, v, (char *)a.QO + row * 128 * osz, 1, f, s);
    if (live && s == 0) {
        const float w = a.W[(int64_t)b * a.ws[0] + (int64_t)head * a.ws[1] + t * a.ws[2]] * a.weight_scale;
        a.WO[row] = w * scale;
    }
}

// ---- keys ------------------------------------------------------------------------------------------------------------------------
struct KRow {
    bool live;
    int b, j;
    int64_t tok;
};

// fa2_decode_append_q.hip's locate at four rows a wave: the row a 16-lane group owns, the new lengths written on the way.
template <bool PK> __device__ __forceinline__ KRow locate(const Fa2AppendQProblem &a) {
    KRow r = {false, 0, 0, 0};
    const int cap = a.capacity;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + threadIdx.y;
    const int64_t slot = wave * 4 + (threadIdx.x >> 4);
    int64_t t;  // the token of its sequence
    if constexpr (PK) {
        const int64_t flat = wave * 64 + threadIdx.x;  // one thread per sequence, sequences without tokens included
        if (flat < a.B) {
            int st0, n, st = a.seqlens[flat];
            fa2_varlen_seq(a.cu_new, (int)flat, a.total_new, a.max_new, st0, n);
            st = st < 0 ? 0 : (st > cap ? cap : st);
            a.seqlens_out[flat] = st + n < cap ? st + n : cap;  // st + n <= 2^29
        }
        if (slot >= a.total_new) return r;
        int st0, n;
        if (!fa2_varlen_owner(a.cu_new, a.B, a.total_new, a.max_new, (int)slot, r.b, st0, n)) return r;
        t = slot - st0;
    } else {
        r.b = blockIdx.z;
        t = slot;
    }
    int start = a.seqlens[r.b];
    start = start < 0 ? 0 : (start > cap ? cap : start);
    if constexpr (!PK) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
            const int n = start + a.N_new;  // <= 2^29
            a.seqlens_out[r.b] = n < cap ? n : cap;
        }
        if (t >= a.N_new) return r;
    }
    if (start + t >= cap) return r;  // past the capacity: dropped
    r.j = start + (int)t;
    r.tok = slot;
    r.live = true;
    return r;
}

template <class E, int OUT, bool PK>
__global__ __launch_bounds__(64 * kWaves) void fa2_indexer_prep_k_kernel(const Fa2AppendQProblem a, const PrepForm f) {
    constexpr int64_t csz = OUT == 0 ? 2 : 1;  // bytes per unit of the cache's strides
    const int s = threadIdx.x & 15;
    const KRow r = locate<PK>(a);  // (returns a value for every lane: no lane leaves before the exchanges)
    const char *src = nullptr;
    char *dst = nullptr;
    float *sc = nullptr;
    RowRot rr = {nullptr, nullptr, a.rotary_dim, a.interleaved != 0};
    if (r.live) {
        int64_t blk = r.b, row = r.j;  // < capacity <= 2^28
        if (a.table) {
            blk = fa2_decode_page(a.table, (int64_t)r.b * a.table_stride + r.j / a.page_size, a.num_blocks);
            row = r.j % a.page_size;
        }
        src = (const char *)a.src + ((int64_t)r.b * a.sns[0] + r.tok * a.sns[2]) * 2;
        dst = (char *)a.cache + (blk * a.cs[0] + row * a.cs[2]) * csz;
        if constexpr (OUT != 0) sc = a.scale + blk * a.scs[0] + row * a.scs[1];
    }
    if (a.cos) {  // (uniform; a group without a row takes table row 0 and rotates nothing)
        const int64_t pos = r.live ? (r.j < a.S_rot ? r.j : a.S_rot - 1) : 0;  // clamped: no length can read outside the tables
        rr.cosr = (const char *)a.cos + pos * a.cos_stride * 2;
        rr.sinr = (const char *)a.sin + pos * a.sin_stride * 2;
    }
    float v[8];
    transform_row<E>(r.live, src, rr, f, s, v);
    const float scale = store_row<E, OUT>(r.live, v, dst, a.cds, f, s);
    if constexpr (OUT != 0)
        if (r.live && s == 0) *sc = scale;
}

#pragma clang fp contract(fast)

bool aligned(const void *p, int64_t n) { return ((uintptr_t)p & (uintptr_t)(n - 1)) == 0; }
bool rows8(const int64_t *s, int n) {
    for (int k = 0; k < n; ++k)
        if (s[k] % 8 != 0) return false;
    return true;
}

// The exchange path of the rotation: tables of 16-byte aligned rows and a rotary_dim whose units are whole lanes -- and, in the half
// pairing, whose partner lane is an xor away.
bool rot_fast(const void *cos, const void *sin, int64_t cs, int64_t ss, int rd, int interleaved) {
    if (!cos || cs % 8 != 0 || ss % 8 != 0 || !aligned(cos, 16) || !aligned(sin, 16)) return false;
    return interleaved ? rd % 16 == 0 : (rd == 16 || rd == 32 || rd == 64 || rd == 128);
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("%s kernel launch failed: %s", what, hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <class E, int OUT> int launch_q(const Fa2IndexerPrepProblem &p, const PrepForm &f) {
    const dim3 block(64, kWaves);
    const unsigned tiles = (unsigned)((p.H + kRows - 1) / kRows);
    if (p.cu_q) hipLaunchKernelGGL((fa2_indexer_prep_q_kernel<E, OUT, true>), dim3((unsigned)p.total_q, tiles), block, 0, p.stream, p, f);
    else hipLaunchKernelGGL((fa2_indexer_prep_q_kernel<E, OUT, false>), dim3((unsigned)((int64_t)p.B * p.N_q), tiles), block, 0, p.stream, p, f);
    return launched("indexer query preparation");
}

template <class E, int OUT> int launch_k(const Fa2AppendQProblem &p, const PrepForm &f) {
    const dim3 block(64, kWaves);
    if (p.cu_new) {  // flat over the packed rows; the first B threads of the grid write the lengths
        const int64_t nr = ((int64_t)p.total_new + kRows - 1) / kRows, lens = ((int64_t)p.B + 64 * kWaves - 1) / (64 * kWaves);
        hipLaunchKernelGGL((fa2_indexer_prep_k_kernel<E, OUT, true>), dim3((unsigned)(nr > lens ? nr : lens)), block, 0, p.stream, p, f);
    } else {
        const dim3 grid((unsigned)(((int64_t)p.N_new + kRows - 1) / kRows), 1, (unsigned)p.B);
        hipLaunchKernelGGL((fa2_indexer_prep_k_kernel<E, OUT, false>), grid, block, 0, p.stream, p, f);
    }
    return launched("indexer key preparation");
}

// out: the fp8 format written, or 0 for the rows' own dtype
template <class E> int launch_q_out(int32_t out, const Fa2IndexerPrepProblem &p, const PrepForm &f) {
    if (out == FA2_DTYPE_F8E4M3) return launch_q<E, FA2_DTYPE_F8E4M3>(p, f);
    if (out == FA2_DTYPE_F8E5M2) return launch_q<E, FA2_DTYPE_F8E5M2>(p, f);
    return launch_q<E, 0>(p, f);
}
template <class E> int launch_k_out(int32_t out, const Fa2AppendQProblem &p, const PrepForm &f) {
    if (out == FA2_DTYPE_F8E4M3) return launch_k<E, FA2_DTYPE_F8E4M3>(p, f);
    if (out == FA2_DTYPE_F8E5M2) return launch_k<E, FA2_DTYPE_F8E5M2>(p, f);
    return launch_k<E, 0>(p, f);
}

}  // namespace

int fa2_launch_indexer_prep_q(const Fa2IndexerPrepProblem &p) {
    PrepForm f;
    f.src_vec = rows8(p.qs, 3) && aligned(p.Q, 16);
    f.dst_vec = 1;  // q_out is contiguous and 16-byte aligned (checked)
    f.rot_fast = rot_fast(p.cos, p.sin, p.cos_stride, p.sin_stride, p.rotary_dim, p.interleaved);
    f.hadamard = p.hadamard;
    const int32_t out = p.out_dtype == p.dtype ? 0 : p.out_dtype;
    if (p.dtype == FA2_DTYPE_F16) return launch_q_out<AppF16>(out, p, f);
    if (p.dtype == FA2_DTYPE_BF16) return launch_q_out<AppBF16>(out, p, f);
    fa2_set_error("indexer query preparation: dtype enum %d is not supported", p.dtype);
    return FA2_ERR_UNSUPPORTED;
}

int fa2_launch_indexer_prep_k(const Fa2AppendQProblem &p, bool hadamard) {
    const bool fp8 = p.mode == FA2_APPENDQ_IDX8;
    PrepForm f;
    f.src_vec = rows8(p.sns, 3) && aligned(p.src, 16);
    f.dst_vec = p.cds == 1 && rows8(p.cs, 3) && aligned(p.cache, fp8 ? 8 : 16);
    f.rot_fast = rot_fast(p.cos, p.sin, p.cos_stride, p.sin_stride, p.rotary_dim, p.interleaved);
    f.hadamard = hadamard;
    const int32_t out = fp8 ? p.cache_dtype : 0;
    if (p.dtype == FA2_DTYPE_F16) return launch_k_out<AppF16>(out, p, f);
    if (p.dtype == FA2_DTYPE_BF16) return launch_k_out<AppBF16>(out, p, f);
    fa2_set_error("indexer key preparation: dtype enum %d is not supported", p.dtype);
    return FA2_ERR_UNSUPPORTED;
}
