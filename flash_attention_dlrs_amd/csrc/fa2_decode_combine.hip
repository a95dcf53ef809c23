// fa2_decode_combine.hip -- second launch of a split KV-cache decode (fa2_fwd_kvcache with num_splits > 1): merges the fp32
// partials the split kernels left in the workspace, one (b, h, q) row per wave, in fp32:
//
//     m = max_s L_s,   w_s = 2^(L_s - m),   O = sum_s w_s O_s / sum_s w_s,   L = m + log2 sum_s w_s
//
// and O = 0, L = +inf when every split is empty (all L_s = -inf).  It is a launch of its own on the caller's stream: the kernel
// boundary is what makes the partials of workgroups on other XCDs (whose L2s are not coherent with each other) visible.
#include <math.h>

#include "fa2_decode.h"
#include "fa2_elem.h"

namespace {

constexpr int kRowsPerBlock = 4;  // one wave each

struct CombineArgs {
    void *O, *L;
    int64_t os[4], ls[2];
    const float *o_part, *l_part;
    int64_t rows;  // B * H * N_q
    int H, N_q, d, num_splits;
};

template <class E> __global__ __launch_bounds__(kRowsPerBlock * 64) void fa2_decode_combine_kernel(const CombineArgs a) {
    using A = typename E::acc_t;
    __shared__ float w_lds[kRowsPerBlock][FA2_KVCACHE_MAX_SPLITS];  // the weights of a row, computed once
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
    const bool live = row < a.rows;  // (no early return: one barrier below)

    // lane owns splits lane and lane + 64 (num_splits <= 128)
    float l0 = -INFINITY, l1 = -INFINITY;
    if (live && lane < a.num_splits) l0 = a.l_part[(int64_t)lane * a.rows + row];
    if (live && lane + 64 < a.num_splits) l1 = a.l_part[(int64_t)(lane + 64) * a.rows + row];
    float m = fmaxf(l0, l1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const bool seen = m != -INFINITY;  // else no split saw a visible key
    const float w0 = seen ? exp2f(l0 - m) : 0.0f, w1 = seen ? exp2f(l1 - m) : 0.0f;
    float wsum = w0 + w1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o, 64);
    w_lds[wave][lane] = w0;
    w_lds[wave][lane + 64] = w1;
    __syncthreads();
    if (!live) return;

    const int q = (int)(row % a.N_q);
    const int64_t bh = row / a.N_q;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const int64_t o_off = b * a.os[0] + h * a.os[1] + (int64_t)q * a.os[2];
    const float inv = seen ? 1.0f / wsum : 0.0f;
    for (int x = lane; x < a.d; x += 64) {
        float acc = 0.0f;
        if (seen)
            for (int s = 0; s < a.num_splits; ++s) acc += w_lds[wave][s] * a.o_part[((int64_t)s * a.rows + row) * a.d + x];
        E::store(a.O, o_off + (int64_t)x * a.os[3], (A)(acc * inv));
    }
    if (lane == 0) E::store(a.L, b * a.ls[0] + h * a.ls[1] + q, seen ? (A)(m + log2f(wsum)) : (A)INFINITY);
}

template <class E> int launch_e(const Fa2DecodeProblem &p, const CombineArgs &a) {
    const int64_t nblk = (a.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    if (nblk > 0x7fffffffLL) {
        fa2_set_error("kvcache combine: grid too large");
        return FA2_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL((fa2_decode_combine_kernel<E>), dim3((unsigned)nblk), dim3(kRowsPerBlock * 64), 0, p.stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fa2_set_error("kvcache combine kernel launch failed: %s", hipGetErrorString(e));
        return FA2_ERR_LAUNCH;
    }
    return FA2_OK;
}

}  // namespace

int fa2_launch_decode_combine(const Fa2DecodeProblem &p) {
    CombineArgs a;
    a.O = p.O; a.L = p.L;
    for (int k = 0; k < 4; ++k) a.os[k] = p.os[k];
    a.ls[0] = p.ls[0]; a.ls[1] = p.ls[1];
    a.o_part = p.o_part; a.l_part = p.l_part;
    a.rows = (int64_t)p.B * p.H * p.N_q;
    a.H = p.H; a.N_q = p.N_q; a.d = p.d; a.num_splits = p.num_splits;
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32>(p, a);
    case FA2_DTYPE_F16: return launch_e<ElemF16>(p, a);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16>(p, a);
    case FA2_DTYPE_F64: return launch_e<ElemF64>(p, a);
    default: fa2_set_error("kvcache: dtype enum %d is not supported", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}
