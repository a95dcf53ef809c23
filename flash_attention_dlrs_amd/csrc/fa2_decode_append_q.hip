// fa2_decode_append_q.hip -- the QUANTISING cache writers (include/fa2_fwd.h): fa2_kvcache_mla_append_ds / _varlen_ds put new latent
// rows into the tile-scaled fp8 cache (656-byte rows: 512 e4m3 bytes, 4 fp32 tile scales, 64 rotary columns in 16 bits),
// fa2_mla_indexer_append / _varlen put index keys into the indexer's fp8 cache with one power-of-two scale per row (or copy them into a
// cache of their own dtype).  One launch each, lengths included.
//
// Why not fa2_decode_append.hip: there a lane owns its units of a row and never talks to another lane.  Here a byte depends on the
// maximum of 128 (or d_I) columns, so a GROUP OF LANES owns a row, each lane keeps its columns in registers between the reduction and
// the quantisation (a row is read once), and the maximum crosses lanes by shuffles inside the group.  No LDS, no barrier.
//
// Work layout.  A block is 4 waves (dim3(64, 4)); a wave owns one row, or four in the index keys' vector form.
//   fp8_ds, vector form: lane l loads the 16 bytes that are latent columns 8 l .. 8 l + 7, so tile t (columns 128 t .. 128 t + 127) is
//     lanes 16 t .. 16 t + 15 -- one DPP row.  amax: 8 fmaxf(|x|) in the lane, then xor-shuffles by 1, 2, 4, 8, which stay inside
//     those 16 lanes.  Every lane then holds its tile's scale, quantises its 8 values and stores one uint2: the wave writes 512
//     contiguous bytes.  Lanes with (l & 15) == 0 store the four scales.  Lanes 0 .. 7 carry the 64 rotary columns, 16 bytes each; in
//     the half pairing the partner unit sits rotary_dim / 16 lanes away and comes by a shuffle, in the interleaved pairing it is in
//     the lane.  They store 16 bytes at 528 + 16 l where the row is 16-byte aligned, else two 8-byte halves.
//   fp8_ds, element form: the same lane map, one element at a time with any strides and alignment; byte stores, the same bytes.
//   index keys, vector form (d_I = 128): 16 lanes of 8 columns are a row, a wave holds four; the same 16-lane reduction.
//   index keys, general form (d_I <= 576): a wave per row, lane l owns columns l, l + 64, ... (at most 9, kept in registers), the
//     reduction runs over the wave.  The same-dtype cache takes this form without the reduction: a copy of bits.
// The fixed forms map blocks to (token tile, KV head, sequence); the packed forms run flat over the packed rows and find a row's
// sequence with fa2_varlen_owner, as fa2_decode_append.hip's packed form does, and write the lengths as that kernel writes them.
//
// Arithmetic (pinned to torch: quantize_mla_cache_ds, quantize_index_keys; the tests compare bits).  fp8_ds: scale =
// __fdiv_rn(fmaxf(amax, 1e-4f), 448), byte = e4m3(clamp(__fdiv_rn(x, scale), +-448)) with fa2_append_arith.h's helpers; the rotary
// columns are the 16-bit latent append's (rot_pair, one rounding to the dtype).  Index keys: q = __fdiv_rn(amax, top) = m 2^e with m
// in [0.5, 1); the scale is 2^e, or 2^(e - 1) at m = 0.5, read off q's bits, 1 for a row of zeros; byte = fp8(clamp(x / scale)).
//
// Every result leaves through ordinary vector stores.
#include "fa2_decode.h"
#include "fa2_append_arith.h"

namespace {

constexpr int kWaves = 4;

// The row a lane group owns: sequence b, packed or per-sequence token `tok` (the row of the sources), key index j.  live: there is one.
struct QRow {
    bool live;
    int b, j;
    int64_t tok;
};

// RPW rows per wave (1, or 4 groups of 16 lanes).  Writes the new lengths on the way, as fa2_decode_append_kernel does.
template <bool PK, int RPW> __device__ __forceinline__ QRow locate(const Fa2AppendQProblem &a) {
    QRow r = {false, 0, 0, 0};
    const int cap = a.capacity;
    const int64_t wave = (int64_t)blockIdx.x * kWaves + threadIdx.y;
    const int64_t slot = wave * RPW + (RPW > 1 ? (int)(threadIdx.x >> 4) : 0);
    int64_t t;  // the token of its sequence
    if constexpr (PK) {
        if (blockIdx.y == 0) {  // one thread per sequence, sequences without tokens included
            const int64_t flat = wave * 64 + threadIdx.x;
            if (flat < a.B) {
                int s, n, st = a.seqlens[flat];
                fa2_varlen_seq(a.cu_new, (int)flat, a.total_new, a.max_new, s, n);
                st = st < 0 ? 0 : (st > cap ? cap : st);
                a.seqlens_out[flat] = st + n < cap ? st + n : cap;  // st + n <= 2^29
            }
        }
        if (slot >= a.total_new) return r;
        int s, n;
        if (!fa2_varlen_owner(a.cu_new, a.B, a.total_new, a.max_new, (int)slot, r.b, s, n)) return r;
        t = slot - s;
    } else {
        r.b = blockIdx.z;
        t = slot;
    }
    int start = a.seqlens[r.b];
    start = start < 0 ? 0 : (start > cap ? cap : start);
    if constexpr (!PK) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
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

// The maximum over the 16 lanes of a DPP row: the xor partners 1, 2, 4, 8 never leave it.
__device__ __forceinline__ float row16_max(float m) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

template <int KV> __device__ __forceinline__ uint2 fp8_pack8(const float (&v)[8], float scale) {
    float q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = fp8_scaled<KV>(v[k], scale);
    int lo = fp8_pack2<KV, false>(q[0], q[1], 0), hi = fp8_pack2<KV, false>(q[4], q[5], 0);
    lo = fp8_pack2<KV, true>(q[2], q[3], lo);
    hi = fp8_pack2<KV, true>(q[6], q[7], hi);
    return make_uint2((uint32_t)lo, (uint32_t)hi);
}

template <int KV> __device__ __forceinline__ uint8_t fp8_byte(float x, float scale) {
    return (uint8_t)fp8_pack2<KV, false>(fp8_scaled<KV>(x, scale), 0.0f, 0);
}

__device__ __forceinline__ float ds_scale(float amax) { return __fdiv_rn(fmaxf(amax, 1e-4f), 448.0f); }

// The index keys' scale: the smallest power of two with amax / scale <= top.  q = amax / top = 1.M 2^(E - 127) = m 2^(E - 126) in
// frexp's terms, m = 0.5 exactly when M = 0: the scale's exponent field is E + 1, or E at M = 0.  (A non-finite amax is outside the
// statement; the field is held at 254 so that the scale stays a positive finite number.)
template <int KV> __device__ __forceinline__ float pow2_scale(float amax) {
    constexpr float top = KV == FA2_DTYPE_F8E4M3 ? 448.0f : 57344.0f;
    const uint32_t q = __builtin_bit_cast(uint32_t, __fdiv_rn(amax, top));
    if (q == 0) return 1.0f;
    const uint32_t e = (q >> 23) + ((q & 0x7fffffu) ? 1u : 0u);
    return __builtin_bit_cast(float, (e < 254u ? e : 254u) << 23);
}

// ---- fp8_ds: one wave, one row ---------------------------------------------------------------------------------------------------
// c: column 0 of the latent source row, pe: column 0 of the rotary source row, dst: byte 0 of the cache row, cosr / sinr: the table
// rows of the row's position or null.
template <class E> __device__ __forceinline__ void ds_row_vec(const Fa2AppendQProblem &a, const char *c, const char *pe, char *dst,
                                                              const char *cosr, const char *sinr) {
    const int l = threadIdx.x;
    float v[8];
    widen8<E>(*(const uint4 *)(c + l * 16), v);
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(v[k]));
    const float scale = ds_scale(row16_max(m));
    *(uint2 *)(dst + l * 8) = fp8_pack8<FA2_DTYPE_F8E4M3>(v, scale);
    if ((l & 15) == 0) *(float *)(dst + kFa2DsScaleOff + (l >> 4) * 4) = scale;

    // the rotary columns: lane l < 8 holds columns 8 l .. 8 l + 7 of the 64
    const bool mine = l < 8;
    uint4 xu = make_uint4(0, 0, 0, 0);
    if (mine) xu = *(const uint4 *)(pe + l * 16);
    if (cosr) {  // (uniform over the wave)
        const int rd = a.rotary_dim, rcol = l * 8;
        const bool rot = mine && rcol < rd;  // rd % 16 == 0: a unit is inside the rotary range or outside it
        float x[8];
        widen8<E>(xu, x);
        if (a.interleaved) {  // pairs (2i, 2i + 1) inside the unit, table columns rcol / 2 .. rcol / 2 + 3
            if (rot) {
                const uint2 cu = *(const uint2 *)(cosr + rcol), su = *(const uint2 *)(sinr + rcol);
                const uint32_t cw[2] = {cu.x, cu.y}, sw[2] = {su.x, su.y};
                float o[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float cc = E::widen((uint16_t)(k & 1 ? cw[k >> 1] >> 16 : cw[k >> 1] & 0xffffu));
                    const float ss = E::widen((uint16_t)(k & 1 ? sw[k >> 1] >> 16 : sw[k >> 1] & 0xffffu));
                    o[2 * k] = rot_pair<float>(x[2 * k], x[2 * k + 1], cc, ss, true);
                    o[2 * k + 1] = rot_pair<float>(x[2 * k + 1], x[2 * k], cc, ss, false);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = o[k];
            }
        } else {  // column i with i + rd / 2: the partner unit is rd / 16 lanes away
            const int half = rd >> 1;
            const bool first = rcol < half;
            const int from = rot ? (first ? l + (rd >> 4) : l - (rd >> 4)) : l;  // in [0, 8) for the lanes that rotate
            const uint4 yu = make_uint4(__shfl(xu.x, from, 64), __shfl(xu.y, from, 64), __shfl(xu.z, from, 64), __shfl(xu.w, from, 64));
            if (rot) {
                const int ci = first ? rcol : rcol - half;
                float y[8], cs[8], sn[8];
                widen8<E>(yu, y);
                widen8<E>(*(const uint4 *)(cosr + ci * 2), cs);
                widen8<E>(*(const uint4 *)(sinr + ci * 2), sn);
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = rot_pair<float>(x[k], y[k], cs[k], sn[k], first);
            }
        }
        if (rot) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (uint32_t)E::narrow(x[2 * k]) | ((uint32_t)E::narrow(x[2 * k + 1]) << 16);
            xu = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    if (mine) {
        char *o = dst + kFa2DsRopeOff + l * 16;  // the row is 8-byte aligned, 528 = 16 * 33
        if (((uintptr_t)o & 15) == 0) *(uint4 *)o = xu;
        else { *(uint2 *)o = make_uint2(xu.x, xu.y); *(uint2 *)(o + 8) = make_uint2(xu.z, xu.w); }
    }
}

// css / pes: the column strides of c and pe, in elements
template <class E> __device__ __forceinline__ void ds_row_elem(const Fa2AppendQProblem &a, const char *c, int64_t css, const char *pe,
                                                               int64_t pes, char *dst, const char *cosr, const char *sinr) {
    const int l = threadIdx.x;
    float v[8];
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = E::load(c, (int64_t)(8 * l + k) * css);
        m = fmaxf(m, fabsf(v[k]));
    }
    const float scale = ds_scale(row16_max(m));
    uint8_t *out = (uint8_t *)dst;
#pragma unroll
    for (int k = 0; k < 8; ++k) out[8 * l + k] = fp8_byte<FA2_DTYPE_F8E4M3>(v[k], scale);
    if ((l & 15) == 0) {
        const uint32_t sb = __builtin_bit_cast(uint32_t, scale);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[kFa2DsScaleOff + (l >> 4) * 4 + k] = (uint8_t)(sb >> (8 * k));
    }
    // the rotary columns: lane l is column l of the 64
    uint16_t bits = ((const uint16_t *)pe)[(int64_t)l * pes];
    const int rd = a.rotary_dim;
    if (cosr && l < rd) {
        const int half = rd >> 1;
        int partner, ci;
        bool first;
        if (a.interleaved) { first = !(l & 1); partner = l ^ 1; ci = l >> 1; }
        else { first = l < half; partner = first ? l + half : l - half; ci = first ? l : l - half; }
        bits = E::narrow(rot_pair<float>(E::load(pe, (int64_t)l * pes), E::load(pe, (int64_t)partner * pes), E::load(cosr, ci),
                                         E::load(sinr, ci), first));
    }
    out[kFa2DsRopeOff + 2 * l] = (uint8_t)bits;
    out[kFa2DsRopeOff + 2 * l + 1] = (uint8_t)(bits >> 8);
}

// ---- index keys ------------------------------------------------------------------------------------------------------------------
// vector form, d_I = 128: 16 lanes a row.  The shuffles run for every lane of the wave; a group without a row reduces zeros.
template <class E, int KV> __device__ __forceinline__ void idx_row_vec(bool live, const char *src, char *dst, float *sc) {
    const int s = threadIdx.x & 15;
    uint4 xu = make_uint4(0, 0, 0, 0);
    if (live) xu = *(const uint4 *)(src + s * 16);
    float v[8];
    widen8<E>(xu, v);
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(v[k]));
    const float scale = pow2_scale<KV>(row16_max(m));
    if (!live) return;
    *(uint2 *)(dst + s * 8) = fp8_pack8<KV>(v, scale);
    if (s == 0) *sc = scale;
}

constexpr int kIdxCols = 9;  // ceil(576 / 64): the columns of a lane in the general form

template <class E, int KV> __device__ __forceinline__ void idx_row_elem(int d, const char *src, int64_t ss, char *dst, int64_t ds, float *sc) {
    const int l = threadIdx.x;
    float v[kIdxCols];
    float m = 0.0f;
#pragma unroll
    for (int i = 0; i < kIdxCols; ++i) {
        const int c = l + 64 * i;
        v[i] = c < d ? E::load(src, (int64_t)c * ss) : 0.0f;
        m = fmaxf(m, fabsf(v[i]));
    }
    const float scale = pow2_scale<KV>(wave_max(m));
#pragma unroll
    for (int i = 0; i < kIdxCols; ++i) {
        const int c = l + 64 * i;
        if (c < d) ((uint8_t *)dst)[(int64_t)c * ds] = fp8_byte<KV>(v[i], scale);
    }
    if (l == 0) *sc = scale;
}

template <class E> __device__ __forceinline__ void copy_row(int d, const char *src, int64_t ss, char *dst, int64_t ds) {
    using B = typename E::bits_t;
    for (int c = threadIdx.x; c < d; c += 64) ((B *)dst)[(int64_t)c * ds] = ((const B *)src)[(int64_t)c * ss];
}

// MODE: FA2_APPENDQ_*; KV: the fp8 format written (DS: e4m3; COPY: 0); VEC: the vector form; PK: the packed form.
template <class E, int MODE, int KV, bool VEC, bool PK>
__global__ __launch_bounds__(64 * kWaves) void fa2_decode_append_q_kernel(const Fa2AppendQProblem a) {
    constexpr int RPW = MODE == FA2_APPENDQ_IDX8 && VEC ? 4 : 1;
    constexpr int64_t esz = sizeof(typename E::bits_t);
    constexpr int64_t csz = MODE == FA2_APPENDQ_COPY ? esz : 1;  // bytes per unit of the cache's strides
    const QRow r = locate<PK, RPW>(a);
    if constexpr (RPW == 1)
        if (!r.live) return;  // (the whole wave)
    const int hk = blockIdx.y;
    const char *src = nullptr;
    char *dst = nullptr;
    float *sc = nullptr;
    if (r.live) {
        int64_t blk = r.b, row = r.j;  // < capacity <= 2^28
        if (a.table) {
            blk = fa2_decode_page(a.table, (int64_t)r.b * a.table_stride + r.j / a.page_size, a.num_blocks);
            row = r.j % a.page_size;
        }
        src = (const char *)a.src + ((int64_t)r.b * a.sns[0] + (int64_t)hk * a.sns[1] + r.tok * a.sns[2]) * esz;
        dst = (char *)a.cache + (blk * a.cs[0] + (int64_t)hk * a.cs[1] + row * a.cs[2]) * csz;
        if constexpr (MODE == FA2_APPENDQ_IDX8) sc = a.scale + blk * a.scs[0] + row * a.scs[1];
    }
    if constexpr (MODE == FA2_APPENDQ_DS) {
        const char *pe = (const char *)a.src2 + ((int64_t)r.b * a.sns2[0] + (int64_t)hk * a.sns2[1] + r.tok * a.sns2[2]) * esz;
        const char *cosr = nullptr, *sinr = nullptr;
        if (a.cos) {
            const int64_t pos = r.j < a.S_rot ? r.j : a.S_rot - 1;  // clamped: no length can read outside the tables
            cosr = (const char *)a.cos + pos * a.cos_stride * esz;
            sinr = (const char *)a.sin + pos * a.sin_stride * esz;
        }
        if constexpr (VEC) ds_row_vec<E>(a, src, pe, dst, cosr, sinr);
        else ds_row_elem<E>(a, src, a.sns[3], pe, a.sns2[3], dst, cosr, sinr);
    } else if constexpr (MODE == FA2_APPENDQ_IDX8) {
        if constexpr (VEC) idx_row_vec<E, KV>(r.live, src, dst, sc);
        else idx_row_elem<E, KV>(a.d, src, a.sns[3], dst, a.cds, sc);
    } else {
        copy_row<E>(a.d, src, a.sns[3], dst, a.cds);
    }
}

bool aligned(const void *p, int64_t n) { return ((uintptr_t)p & (uintptr_t)(n - 1)) == 0; }
bool rows8(const int64_t *s, int n) {
    for (int k = 0; k < n; ++k)
        if (s[k] % 8 != 0) return false;
    return true;
}

// The vector forms: 16-bit sources with unit column strides and 16-byte aligned rows, cache rows aligned to their 8-byte stores;
// fp8_ds: tables of 16-byte aligned rows and rotary_dim % 16 == 0 as well; index keys: d_I = 128 and unit cache columns.
bool vector_form(const Fa2AppendQProblem &p) {
    if (p.dtype != FA2_DTYPE_F16 && p.dtype != FA2_DTYPE_BF16) return false;
    if (p.sns[3] != 1 || !rows8(p.sns, 3) || !aligned(p.src, 16) || !rows8(p.cs, 3) || !aligned(p.cache, 8)) return false;
    if (p.mode == FA2_APPENDQ_IDX8) return p.d == 128 && p.cds == 1;
    if (p.mode != FA2_APPENDQ_DS) return false;
    if (p.sns2[3] != 1 || !rows8(p.sns2, 3) || !aligned(p.src2, 16)) return false;
    if (p.cos && (p.rotary_dim % 16 != 0 || p.cos_stride % 8 != 0 || p.sin_stride % 8 != 0 || !aligned(p.cos, 16) || !aligned(p.sin, 16)))
        return false;
    return true;
}

template <class E, int MODE, int KV, bool VEC> int launch_form(const Fa2AppendQProblem &p) {
    constexpr int rows = kWaves * (MODE == FA2_APPENDQ_IDX8 && VEC ? 4 : 1);  // per block
    const dim3 block(64, kWaves);
    if (p.cu_new) {  // flat over the packed rows; the first B threads of the blockIdx.y == 0 blocks write the lengths
        const int64_t nr = ((int64_t)p.total_new + rows - 1) / rows, lens = ((int64_t)p.B + 64 * kWaves - 1) / (64 * kWaves);
        const dim3 grid((unsigned)(nr > lens ? nr : lens), (unsigned)p.H_kv);
        hipLaunchKernelGGL((fa2_decode_append_q_kernel<E, MODE, KV, VEC, true>), grid, block, 0, p.stream, p);
    } else {
        const dim3 grid((unsigned)(((int64_t)p.N_new + rows - 1) / rows), (unsigned)p.H_kv, (unsigned)p.B);
        hipLaunchKernelGGL((fa2_decode_append_q_kernel<E, MODE, KV, VEC, false>), grid, block, 0, p.stream, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("quantising append kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

template <class E> int launch_quant(const Fa2AppendQProblem &p) {
    const bool vec = vector_form(p);
    if (p.mode == FA2_APPENDQ_DS)
        return vec ? launch_form<E, FA2_APPENDQ_DS, FA2_DTYPE_F8E4M3, true>(p) : launch_form<E, FA2_APPENDQ_DS, FA2_DTYPE_F8E4M3, false>(p);
    if (p.cache_dtype == FA2_DTYPE_F8E4M3)
        return vec ? launch_form<E, FA2_APPENDQ_IDX8, FA2_DTYPE_F8E4M3, true>(p) : launch_form<E, FA2_APPENDQ_IDX8, FA2_DTYPE_F8E4M3, false>(p);
    return vec ? launch_form<E, FA2_APPENDQ_IDX8, FA2_DTYPE_F8E5M2, true>(p) : launch_form<E, FA2_APPENDQ_IDX8, FA2_DTYPE_F8E5M2, false>(p);
}

}  // namespace

int fa2_launch_decode_append_q(const Fa2AppendQProblem &p) {
    if (p.mode == FA2_APPENDQ_COPY) {  // bits only: f16 and bf16 are one form
        if (p.dtype == FA2_DTYPE_F32) return launch_form<AppF32, FA2_APPENDQ_COPY, 0, false>(p);
        if (p.dtype == FA2_DTYPE_F16 || p.dtype == FA2_DTYPE_BF16) return launch_form<AppF16, FA2_APPENDQ_COPY, 0, false>(p);
    } else {
        if (p.dtype == FA2_DTYPE_F16) return launch_quant<AppF16>(p);
        if (p.dtype == FA2_DTYPE_BF16) return launch_quant<AppBF16>(p);
    }
    fa2_set_error("quantising append: dtype enum %d is not supported", p.dtype);
    return FA2_ERR_UNSUPPORTED;
}
