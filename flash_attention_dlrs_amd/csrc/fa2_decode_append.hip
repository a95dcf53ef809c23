// fa2_decode_append.hip -- the write side of a decode step (fa2_kvcache_append, fa2_kvcache_append_varlen, include/fa2_fwd.h): one
// launch that puts the new tokens' K and V into the cache (contiguous or paged, 16-bit / f32 / f64 or fp8), applies rotary embedding
// to K and to Q, and writes the new lengths.  The decode kernels that follow read seqlens_out as their cache_seqlens and q_rot as
// their Q, so they need no new parameter.
//
// Work layout (the fixed form; the packed form of fa2_kvcache_append_varlen is described at the kernel).  blockIdx.z is the
// sequence, blockIdx.y walks the row slabs of that sequence (H_kv slabs of K, H_kv of V, H of Q when Q is rotated), blockIdx.x the
// tokens: a block is blockDim.y tokens of blockDim.x lanes, lane x owning the units x, x + blockDim.x, ... of its row.  A unit is
// 8 columns (vector path: 16-byte loads, 16- or 8-byte stores) or one column (element path).  No index is ever divided: the host
// picks blockDim.x as the power of two that covers a row (at most 64).
//
// Arithmetic (pinned: flash_attention_wrappers.apply_rotary restates it in torch and the tests compare bits).  Inputs are widened to
// fp32 (f64 stays f64); o1 = x1 c - x2 s and o2 = x2 c + x1 s with each product and the sum or difference rounded separately -- the
// helpers below sit under `#pragma clang fp contract(off)`, because hipcc contracts a * b - c * d into an FMA by default and the
// __fmul_rn / __fsub_rn spellings are plain operators in its headers, which contract just the same; one rounding to nearest even to
// the cache dtype.  For an fp8 cache the fp32 value (not rounded to 16 bits in between) is divided by the descale with the correctly
// rounded division, clamped to +-finfo.max and converted by v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 (OCP formats on gfx950, nearest even).
// Columns outside the rotary range, and V, are copied bit for bit into a cache of their own dtype.
//
// The latent form (LAT: fa2_kvcache_mla_append, fa2_kvcache_mla_append_varlen) writes the one tensor of an MLA cache: there are no V
// slabs (the value is a view of the same row), a row's columns [0, d_v) come from c_new and [d_v, d) from pe_new, each with a pointer
// and strides of its own, and the rotary range starts at column d_v -- of the cache row and of Q alike.  Inside that range the
// pairing, the tables and the arithmetic are the ones above; one descale (kd) scales the whole row.
//
// Every result leaves through ordinary vector stores.
#include "fa2_decode.h"
#include "fa2_elem.h"

namespace {

// ---- the pinned arithmetic -------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
// One output of a rotary pair: `x` is the column being written, `y` its partner; `first` is the x1 side (o1 = x1 c - x2 s), else
// the x2 side (o2 = x2 c + x1 s).
template <class T> __device__ __forceinline__ T rot_pair(T x, T y, T c, T s, bool first) {
    const T xc = x * c;
    const T ys = y * s;
    return first ? xc - ys : xc + ys;
}
#pragma clang fp contract(fast)

template <int KV> __device__ __forceinline__ float fp8_scaled(float x, float ds) {
    constexpr float top = KV == FA2_DTYPE_F8E4M3 ? 448.0f : 57344.0f;
    return fminf(fmaxf(__fdiv_rn(x, ds), -top), top);
}
// two fp32 -> two fp8 bytes in the low (hi = false) or high half of `old`
template <int KV, bool HI> __device__ __forceinline__ int fp8_pack2(float a, float b, int old) {
    if constexpr (KV == FA2_DTYPE_F8E4M3) return __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, HI);
    else return __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, HI);
}

struct Row {          // one row of d columns to process, uniform over the lanes of a row
    const char *src;  // element 0 of the input row
    char *dst;        // element 0 of the output row
    int64_t ss, ds;   // d-strides of src and dst, in elements (element path)
    // LAT only: columns >= off are read from src2 (the element that becomes column off) with d-stride ss2, and rotated from off on
    const char *src2;
    int64_t ss2;
    int off;
    const char *cos, *sin;  // the table rows of this row's position, or null: no rotary
    float descale;    // fp8 output only
};

// ---- element path: one column per unit, any strides, any dtype -------------------------------------------------------------------
// OUT = 0: the output has E's dtype; FA2_DTYPE_F8E4M3 / FA2_DTYPE_F8E5M2: an fp8 cache.
// The input element that becomes column c.
template <class E, bool LAT> __device__ __forceinline__ const char *col_src(const Row &r, int c) {
    constexpr int64_t esz = sizeof(typename E::bits_t);
    if constexpr (LAT)
        if (c >= r.off) return r.src2 + (int64_t)(c - r.off) * r.ss2 * esz;
    return r.src + (int64_t)c * r.ss * esz;
}

template <class E, int OUT, bool LAT> __device__ __forceinline__ void unit_elem(const Row &r, int c, int rd, int interleaved) {
    using T = typename E::acc_t;  // float, or double for f64
    T v;
    const int off = LAT ? r.off : 0;
    const int rc = c - off;  // the column inside the rotary range
    const bool rot = r.cos && rc >= 0 && rc < rd;
    if (rot) {
        const int half = rd >> 1;
        int partner, ci;
        bool first;
        if (interleaved) { first = !(rc & 1); partner = rc ^ 1; ci = rc >> 1; }
        else { first = rc < half; partner = first ? rc + half : rc - half; ci = first ? rc : rc - half; }
        v = rot_pair<T>(E::load(col_src<E, LAT>(r, c), 0), E::load(col_src<E, LAT>(r, partner + off), 0), E::load(r.cos, ci),
                        E::load(r.sin, ci), first);
    } else if constexpr (OUT == 0) {  // a copy, bit for bit
        using B = typename E::bits_t;
        ((B *)r.dst)[(int64_t)c * r.ds] = *(const B *)col_src<E, LAT>(r, c);
        return;
    } else {
        v = E::load(col_src<E, LAT>(r, c), 0);
    }
    if constexpr (OUT == 0) E::store(r.dst, (int64_t)c * r.ds, v);
    else ((uint8_t *)r.dst)[(int64_t)c * r.ds] = (uint8_t)fp8_pack2<OUT, false>(fp8_scaled<OUT>((float)v, r.descale), 0.0f, 0);
}

// ---- vector path: 8 columns per unit, f16 / bf16 input, unit d-strides, aligned rows, rotary_dim % 16 == 0 -----------------------
// (LAT: off % 8 == 0 as well, so a unit lies in one source, and the rotary range, which starts at off, lies in src2)
template <class E> __device__ __forceinline__ void widen8(const uint4 &u, float (&f)[8]) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = E::widen((uint16_t)(w[k] & 0xffffu));
        f[2 * k + 1] = E::widen((uint16_t)(w[k] >> 16));
    }
}

template <class E, int OUT, bool LAT> __device__ __forceinline__ void unit_vec(const Row &r, int c, int rd, int interleaved) {
    const int col = c * 8;
    const int rcol = LAT ? col - r.off : col;                 // the column inside the rotary range
    const char *rsrc = LAT ? r.src2 : r.src;                  // ... and the source that holds the range
    const uint4 xu = *(const uint4 *)(rcol >= 0 ? rsrc + (int64_t)rcol * 2 : r.src + (int64_t)col * 2);
    const bool rot = r.cos && rcol >= 0 && rcol < rd;  // rd % 16 == 0: a unit is inside the rotary range or outside it
    if (!rot && OUT == 0) {
        *(uint4 *)(r.dst + (int64_t)col * 2) = xu;
        return;
    }
    float v[8];
    widen8<E>(xu, v);
    if (rot) {
        float cs[8], sn[8];
        if (interleaved) {  // pairs (2i, 2i + 1) inside the unit, table columns col / 2 .. col / 2 + 3
            const uint2 cu = *(const uint2 *)(r.cos + (int64_t)rcol), su = *(const uint2 *)(r.sin + (int64_t)rcol);
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
        } else {  // column i with i + rd / 2: the partner unit is rd / 16 units away
            const int half = rd >> 1;
            const bool first = rcol < half;
            const int pcol = first ? rcol + half : rcol - half, ci = first ? rcol : rcol - half;
            float y[8];
            widen8<E>(*(const uint4 *)(rsrc + (int64_t)pcol * 2), y);
            widen8<E>(*(const uint4 *)(r.cos + (int64_t)ci * 2), cs);
            widen8<E>(*(const uint4 *)(r.sin + (int64_t)ci * 2), sn);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = rot_pair<float>(v[k], y[k], cs[k], sn[k], first);
        }
    }
    if constexpr (OUT == 0) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (uint32_t)E::narrow(v[2 * k]) | ((uint32_t)E::narrow(v[2 * k + 1]) << 16);
        *(uint4 *)(r.dst + (int64_t)col * 2) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = fp8_scaled<OUT>(v[k], r.descale);
        int lo = fp8_pack2<OUT, false>(v[0], v[1], 0), hi = fp8_pack2<OUT, false>(v[4], v[5], 0);
        lo = fp8_pack2<OUT, true>(v[2], v[3], lo);
        hi = fp8_pack2<OUT, true>(v[6], v[7], hi);
        *(uint2 *)(r.dst + (int64_t)col) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
}

// The element types of this kernel: fa2_elem.h's load / store plus the raw 16-bit conversions of the vector path.
struct AppF64 : ElemF64 { using bits_t = uint64_t; };
struct AppF32 : ElemF32 { using bits_t = uint32_t; };
struct AppF16 : ElemF16 {
    using bits_t = uint16_t;
    static __device__ __forceinline__ float widen(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
    static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
};
struct AppBF16 : ElemBF16 {
    using bits_t = uint16_t;
    static __device__ __forceinline__ float widen(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
    static __device__ __forceinline__ uint16_t narrow(float x) { return ElemBF16::bits(x); }
};

template <class E, int OUT, bool VEC, bool LAT> __device__ __forceinline__ void do_row(const Row &r, int units, int rd, int interleaved) {
    for (int c = threadIdx.x; c < units; c += blockDim.x) {
        if constexpr (VEC) unit_vec<E, OUT, LAT>(r, c, rd, interleaved);
        else unit_elem<E, OUT, LAT>(r, c, rd, interleaved);
    }
}

// PK: the packed (ragged) form, fa2_kvcache_append_varlen.  The fixed form's blockIdx.z and its B x N_new token tiles give way to a
// flat layout over the packed rows, so a long chunk beside many one-token decodes launches no empty tiles: blockIdx.x * blockDim.y +
// threadIdx.y is a packed row, which finds its sequence by a binary search over cu_new (once, at most 16 steps: B <= 65535) and
// then checks with fa2_varlen_seq that the sequence owns it -- rows in no sequence do nothing.  Everything after that is the
// fixed form's: the same Row, the same do_row, so the same bytes.
// LAT: the latent form (the head of this file): H_kv slabs of the one cache tensor, then H of Q.
template <class E, int KV, bool VEC, bool PK, bool LAT>
__global__ __launch_bounds__(256) void fa2_decode_append_kernel(const Fa2AppendProblem a) {
    constexpr int64_t esz = sizeof(typename E::bits_t);
    constexpr int64_t csz = KV == 0 ? esz : 1;  // bytes of a cache element
    const int cap = a.capacity;
    int b, start;
    int64_t t;  // this lane's token of sequence b (K, V) or its query row (Q)
    [[maybe_unused]] int64_t row = 0;  // PK: the packed row that token is
    if constexpr (PK) {
        if (blockIdx.y == 0) {  // the new lengths: one thread per sequence, sequences without tokens included
            const int64_t flat = (((int64_t)blockIdx.x * blockDim.y + threadIdx.y) * blockDim.x) + threadIdx.x;
            if (flat < a.B) {
                int s, n, st = a.seqlens[flat];
                fa2_varlen_seq(a.cu_new, (int)flat, a.total_new, a.max_new, s, n);
                st = st < 0 ? 0 : (st > cap ? cap : st);
                a.seqlens_out[flat] = st + n < cap ? st + n : cap;  // st + n <= 2^29
            }
        }
        row = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
        if (row >= a.total_new) return;
        int lo = 0, hi = a.B;  // the last sequence in [0, B) whose clamped offset is <= row (sequence 0 when none is)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            int c = a.cu_new[mid];
            c = c < 0 ? 0 : (c > a.total_new ? a.total_new : c);
            if (c <= row) lo = mid;
            else hi = mid;
        }
        b = lo;
        int s, n;
        fa2_varlen_seq(a.cu_new, b, a.total_new, a.max_new, s, n);
        if (row < s || row >= (int64_t)s + n) return;  // a gap, the surplus of a span past max_new, a row behind the last offset
        t = row - s;  // < n <= max_new <= 2^28
        start = a.seqlens[b];
        start = start < 0 ? 0 : (start > cap ? cap : start);
    } else {
        b = blockIdx.z;
        start = a.seqlens[b];
        start = start < 0 ? 0 : (start > cap ? cap : start);
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
            const int n = start + a.N_new;  // <= 2^29
            a.seqlens_out[b] = n < cap ? n : cap;
        }
        t = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
    }
    const int units = VEC ? a.d >> 3 : a.d;
    const bool rotary = a.cos != nullptr;
    const int nkv = LAT ? a.H_kv : 2 * a.H_kv;
    const int nslab = nkv + (a.Q && rotary ? a.H : 0);
    for (int slab = blockIdx.y; slab < nslab; slab += gridDim.y) {
        Row r;
        if (slab < nkv) {  // a row of K (with rotary) or V (without); LAT: of the latent cache, K's part in every respect
            const bool is_k = LAT || slab < a.H_kv;
            const int hk = is_k ? slab : slab - a.H_kv;
            if constexpr (!PK)
                if (t >= a.N_new) continue;
            if (start + t >= cap) continue;  // past the capacity: dropped
            const int j = start + (int)t;  // the key index this token gets, < capacity <= 2^28
            const int64_t *ns = is_k ? a.kns : a.vns, *cs = is_k ? a.ks : a.vs;
            int64_t off;
            if (a.table) {
                const int page = fa2_decode_page(a.table, (int64_t)b * a.table_stride + j / a.page_size, a.num_blocks);
                off = (int64_t)page * cs[0] + (int64_t)hk * cs[1] + (int64_t)(j % a.page_size) * cs[2];
            } else {
                off = (int64_t)b * cs[0] + (int64_t)hk * cs[1] + (int64_t)j * cs[2];
            }
            if constexpr (PK) r.src = (const char *)(is_k ? a.k_new : a.v_new) + ((int64_t)hk * ns[1] + row * ns[2]) * esz;
            else r.src = (const char *)(is_k ? a.k_new : a.v_new) + ((int64_t)b * ns[0] + (int64_t)hk * ns[1] + t * ns[2]) * esz;
            r.dst = (char *)(is_k ? a.K : a.V) + off * csz;
            r.ss = ns[3];
            r.ds = cs[3];
            if constexpr (LAT) {
                if constexpr (PK) r.src2 = (const char *)a.pe_new + ((int64_t)hk * a.pns[1] + row * a.pns[2]) * esz;
                else r.src2 = (const char *)a.pe_new + ((int64_t)b * a.pns[0] + (int64_t)hk * a.pns[1] + t * a.pns[2]) * esz;
                r.ss2 = a.pns[3];
                r.off = a.d_v;
            }
            r.cos = r.sin = nullptr;
            if (is_k && rotary) {
                const int64_t pos = j < a.S_rot ? j : a.S_rot - 1;  // clamped: no length can read outside the tables
                r.cos = (const char *)a.cos + pos * a.cos_stride * esz;
                r.sin = (const char *)a.sin + pos * a.sin_stride * esz;
            }
            r.descale = 1.0f;
            if constexpr (KV != 0)
                r.descale = is_k ? fa2_decode_descale(a.kd, a.kds[0], a.kds[1], b, hk) : fa2_decode_descale(a.vd, a.vds[0], a.vds[1], b, hk);
            do_row<E, KV, VEC, LAT>(r, units, a.rotary_dim, a.interleaved);
        } else {  // a row of Q, rotated into q_rot, contiguous in Q's dtype: (B, H, N_q, d), or (total_new, H, d) when packed
            const int h = slab - nkv;
            if constexpr (!PK)
                if (t >= a.N_q) continue;
            int64_t pos = start + (a.q_pos_per_row ? t : 0);
            pos = pos < a.S_rot ? pos : a.S_rot - 1;
            if constexpr (PK) {
                r.src = (const char *)a.Q + ((int64_t)h * a.qs[1] + row * a.qs[2]) * esz;
                r.dst = (char *)a.q_rot + ((row * a.H + h) * a.d) * esz;
            } else {
                r.src = (const char *)a.Q + ((int64_t)b * a.qs[0] + (int64_t)h * a.qs[1] + t * a.qs[2]) * esz;
                r.dst = (char *)a.q_rot + ((((int64_t)b * a.H + h) * a.N_q + t) * a.d) * esz;
            }
            r.ss = a.qs[3];
            r.ds = 1;
            if constexpr (LAT) {
                r.src2 = r.src + (int64_t)a.d_v * a.qs[3] * esz;
                r.ss2 = a.qs[3];
                r.off = a.d_v;
            }
            r.cos = (const char *)a.cos + pos * a.cos_stride * esz;
            r.sin = (const char *)a.sin + pos * a.sin_stride * esz;
            r.descale = 1.0f;
            do_row<E, 0, VEC, LAT>(r, units, a.rotary_dim, a.interleaved);
        }
    }
}

bool aligned(const void *p, int64_t n) { return ((uintptr_t)p & (uintptr_t)(n - 1)) == 0; }
bool rows8(const int64_t s[4]) { return s[3] == 1 && s[0] % 8 == 0 && s[1] % 8 == 0 && s[2] % 8 == 0; }

// The vector path: 16-bit inputs, unit d-strides, every row it touches aligned to the width of its loads and stores.  The latent
// form (V null) has pe_new in v_new's place and no 8-column unit across the two sources: d_v % 8 == 0 (and so (d - d_v) % 8 == 0).
bool vector_path(const Fa2AppendProblem &p) {
    if (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16) return false;
    if (p.d % 8 != 0) return false;
    const int64_t cache_align = p.kv_dtype == p.dtype ? 16 : 8;
    if (!p.V) {
        if (p.d_v % 8 != 0 || !rows8(p.kns) || !rows8(p.pns) || !rows8(p.ks)) return false;
        if (!aligned(p.k_new, 16) || !aligned(p.pe_new, 16) || !aligned(p.K, cache_align)) return false;
    } else {
        if (!rows8(p.kns) || !rows8(p.vns) || !rows8(p.ks) || !rows8(p.vs)) return false;
        if (!aligned(p.k_new, 16) || !aligned(p.v_new, 16) || !aligned(p.K, cache_align) || !aligned(p.V, cache_align)) return false;
    }
    if (p.cos) {
        if (p.rotary_dim % 16 != 0 || p.cos_stride % 8 != 0 || p.sin_stride % 8 != 0 || !aligned(p.cos, 16) || !aligned(p.sin, 16))
            return false;
        if (p.Q && (!rows8(p.qs) || !aligned(p.Q, 16) || !aligned(p.q_rot, 16))) return false;
    }
    return true;
}

template <class E, int KV, bool VEC, bool LAT> int launch_form(const Fa2AppendProblem &p) {
    const int units = VEC ? p.d / 8 : p.d;
    int tx = 1;
    while (tx < units && tx < 64) tx *= 2;
    const bool with_q = p.Q && p.cos;
    const int64_t ntok = p.cu_new ? p.total_new : (with_q && p.N_q > p.N_new ? p.N_q : p.N_new);
    int ty = 1;
    while (ty < ntok && tx * ty < 256) ty *= 2;
    const int64_t nslab = (LAT ? 1 : 2) * (int64_t)p.H_kv + (with_q ? p.H : 0);
    if (p.cu_new) {  // flat over the packed rows; the first B threads of the blockIdx.y == 0 blocks write the lengths
        const int64_t rows = (ntok + ty - 1) / ty, lens = ((int64_t)p.B + tx * ty - 1) / (tx * ty);
        const dim3 grid((unsigned)(rows > lens ? rows : lens), (unsigned)(nslab < 65535 ? nslab : 65535));
        hipLaunchKernelGGL((fa2_decode_append_kernel<E, KV, VEC, true, LAT>), grid, dim3(tx, ty), 0, p.stream, p);
    } else {
        const dim3 grid((unsigned)((ntok + ty - 1) / ty), (unsigned)(nslab < 65535 ? nslab : 65535), (unsigned)p.B);
        hipLaunchKernelGGL((fa2_decode_append_kernel<E, KV, VEC, false, LAT>), grid, dim3(tx, ty), 0, p.stream, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache append kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <class E, int KV, bool VEC> int launch(const Fa2AppendProblem &p) {
    return p.V ? launch_form<E, KV, VEC, false>(p) : launch_form<E, KV, VEC, true>(p);
}

template <class E, bool VEC> int launch_kv(const Fa2AppendProblem &p) {
    if (p.kv_dtype == p.dtype) return launch<E, 0, VEC>(p);
    if (p.kv_dtype == FA2_DTYPE_F8E4M3) return launch<E, FA2_DTYPE_F8E4M3, VEC>(p);
    return launch<E, FA2_DTYPE_F8E5M2, VEC>(p);
}

}  // namespace

int fa2_launch_decode_append(const Fa2AppendProblem &p) {
    const bool vec = vector_path(p);
    switch (p.dtype) {
    case FA2_DTYPE_F16: return vec ? launch_kv<AppF16, true>(p) : launch_kv<AppF16, false>(p);
    case FA2_DTYPE_BF16: return vec ? launch_kv<AppBF16, true>(p) : launch_kv<AppBF16, false>(p);
    case FA2_DTYPE_F32: return launch<AppF32, 0, false>(p);
    case FA2_DTYPE_F64: return launch<AppF64, 0, false>(p);
    default: fa2_set_error("kvcache append: dtype enum %d is not supported", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}
