// The gfx950 primitives of the matrix-core kernels: vector types, the MFMA wrappers, the half-wave exchange, LDS-DMA and the
// LDS tile swizzles.  Every matrix-core kernel file (fa2_*mfma*.hip, fa2_decode_mla16.hip) includes this header, and a new one
// starts by including it; nothing here belongs to one kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;

#define LDS_PTR(T) __attribute__((address_space(3))) T *

template <int V> struct IC { static constexpr int value = V; };

// 16-bit matrix products: mfma = v_mfma_f32_32x32x16, mfma16 = v_mfma_f32_16x16x32.
template <typename T> struct Mma;
template <> struct Mma<__bf16> {
    using frag = bf16x8;
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<_Float16> {
    using frag = f16x8;
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

// fp8 matrix products.  E4M3 = true: OCP e4m3fn (v_mfma ... fp8_fp8, v_cvt_pk_fp8_f32); false: e5m2 (bf8).
// mfma = v_mfma_f32_32x32x16 (fa2_mfma8.hip), mfma64 = v_mfma_f32_32x32x64_f8f6f4 (fa2_mfma8x.hip).
template <bool E4M3> struct F8 {
    static __device__ __forceinline__ f32x16 mfma(long a, long b, f32x16 c) {
        if constexpr (E4M3) return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma64(i32x8 a, i32x8 b, f32x16 c) {
        if constexpr (E4M3) return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
        else return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 1, 1, 0, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma_sum(i32x8 a, i32x8 b, f32x4 c) {  // 16x16x128
        if constexpr (E4M3) return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
        else return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 1, 1, 0, 0, 0, 0);
    }
    static constexpr int kOnes = E4M3 ? 0x38383838 : 0x3c3c3c3c;  // four fp8 1.0
    // two floats -> two fp8 (RTNE) into the low (hi = false) or high half of `old`
    template <bool HI> static __device__ __forceinline__ int cvt_pk(float x, float y, int old) {
        if constexpr (E4M3) return __builtin_amdgcn_cvt_pk_fp8_f32(x, y, old, HI);
        else return __builtin_amdgcn_cvt_pk_bf8_f32(x, y, old, HI);
    }
};

// Exchange between the two 32-lane halves of the wave with v_permlane32_swap (VALU, no LDS trip):
// r[0][l] = x[l & 31], r[1][l] = x[32 + (l & 31)].  NB: the elements are copied to scalars before the
// bit cast -- __builtin_bit_cast applied directly to a vector ELEMENT (r[1]) reads element 0 with this
// clang (ROCm 7.2), which silently turned the exchange into a no-op.
__device__ __forceinline__ void half_swap(float x, float &lo, float &hi) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    const unsigned a = r[0], b = r[1];
    lo = __builtin_bit_cast(float, a);
    hi = __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float half_swap_max(float x) {
    float lo, hi;
    half_swap(x, lo, hi);
    return fmaxf(lo, hi);
}
__device__ __forceinline__ float half_swap_sum(float x) {
    float lo, hi;
    half_swap(x, lo, hi);
    return lo + hi;
}

// One LDS-DMA piece: 64 lanes x 16 bytes from (descriptor, per-lane byte offset) to LDS at lds_base + lane*16.
// Inline asm ON PURPOSE: with the builtin, hipcc cannot tell the DMA's destination buffer from the buffer being
// read and puts `s_waitcnt vmcnt(0)` in front of the first ds_read of the V tile -- the transfer then has a
// quarter of an iteration to land instead of a whole one.  The compiler does not see these loads: the
// `s_waitcnt vmcnt(0)` in front of the publishing barrier is ours (dma_wait()).  M0 is saved and restored.
__device__ __forceinline__ void dma16(const i32x4 rsrc, unsigned lds_base, int voffset) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_base), "v"(voffset), "s"(rsrc)
                 : "memory");
}
__device__ __forceinline__ void dma4(const i32x4 rsrc, unsigned lds_base, int voffset) {  // 64 lanes x 4 bytes
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dword %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "s"(lds_base), "v"(voffset), "s"(rsrc)
                 : "memory");
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Chunk swizzle of a row inside a [64][D] 16-bit tile (a function of row & 15 only), and the byte offset of 16-byte
// chunk `ch` of row `row` in that tile.
// D = 128 (256-B rows): chunk ^= ((row&3)<<2 | (row>>2)&3).  A ds_read_b128 lane group reads 16 rows
//   distinct mod 16 at one chunk -> 16 different 16-B slots of the 256-B bank row; a transposed read's
//   half-wave touches rows 4n..4n+3 x one 64-B span -> the (row&3)<<2 term moves each row to its own span.
// D = 64 (128-B rows, two rows per bank row): chunk ^= ((row>>1)&1)<<2 | (row>>2)&3, same argument with
//   row&1 selecting the half of the bank row.
// LDS-DMA writes lane-linearly, so the DMA kernels apply swz through the SOURCE address and again on every read.
template <int D> __device__ __forceinline__ int swz(int row) {
    if constexpr (D == 128) return ((row & 3) << 2) | ((row >> 2) & 3);
    else return (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
}
template <int D> __device__ __forceinline__ int lds_off(int row, int ch) { return row * (D * 2) + ((ch ^ swz<D>(row)) << 4); }

// 16-byte chunk `ch` of row `row` in a [32][D] fp32 tile: chunk ^= row & 15 (low four chunk bits).
template <int D> __device__ __forceinline__ int lds_off32(int row, int ch) { return row * (D * 4) + ((ch ^ (row & 15)) << 4); }

}  // namespace
