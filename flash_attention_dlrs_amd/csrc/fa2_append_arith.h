// The pinned arithmetic of the cache append kernels (fa2_decode_append.hip, fa2_decode_append_q.hip): the rotary pair, the fp8
// quantisation and the raw 16-bit conversions of the vector paths.  flash_attention_wrappers.apply_rotary restates the rotation in
// torch and the tests compare bits, so both kernel files take it from here.
#pragma once
#include "fa2_elem.h"

namespace {

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

// 8 columns of a 16-byte unit, widened
template <class E> __device__ __forceinline__ void widen8(const uint4 &u, float (&f)[8]) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = E::widen((uint16_t)(w[k] & 0xffffu));
        f[2 * k + 1] = E::widen((uint16_t)(w[k] >> 16));
    }
}

// The element types of the append kernels: fa2_elem.h's load / store plus the raw 16-bit conversions of the vector path.
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

}  // namespace
