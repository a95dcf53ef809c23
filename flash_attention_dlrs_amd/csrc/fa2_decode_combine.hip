// fa2_decode_combine.hip -- second launch of a split KV-cache decode (fa2_fwd_kvcache with num_splits > 1): merges the fp32
// partials the split kernels left in the workspace, one (b, h, q) row per wave, in fp32:
//
//     m = max_s L_s,   w_s = 2^(L_s - m),   O = sum_s w_s O_s / sum_s w_s,   L = m + log2 sum_s w_s
//
// and O = 0, L = +inf when every split is empty (all L_s = -inf).  It is a launch of its own on the caller's stream: the kernel
// boundary is what makes the partials of workgroups on other XCDs (whose L2s are not coherent with each other) visible.
//
// Packed queries (fa2_fwd_kvcache_varlen): the partial rows are [total_q * H], row = token * H + head, and only the rows of a
// sequence's own n_q(b) tokens were written.  The grid is (blocks, B): the blocks of sequence b stride over its n_q(b) * H rows,
// so a token outside every sequence is neither read nor written.  The arithmetic of a row is the same.
#include <math.h>

#include "fa2_decode.h"
#include "fa2_elem.h"

namespace {

constexpr int kRowsPerBlock = 4;  // one wave each
constexpr int kPackedBlocks = 1 << 16;  // packed queries: the grid's size, its blocks striding over a sequence's rows

struct CombineArgs {
    void *O, *L;
    int64_t os[4], ls[2];
    const float *o_part, *l_part;
    int64_t rows;  // B * H * N_q
    int H, N_q, d, num_splits;  // d: the columns of O and of the partials (the value head size)
    const int32_t *cu_q;  // packed queries: B + 1 offsets (os[0] = ls[0] = 0), else null
    int total_q, max_q;
};

// One row of the partials, one wave: `row` indexes o_part / l_part, o_off / l_off are the row's element offsets in O and L, w the
// wave's weights in LDS.  Every wave of the block calls it (one barrier inside), dead rows with live = false.
template <class E>
__device__ __forceinline__ void combine_row(const CombineArgs &a, int64_t row, bool live, int64_t o_off, int64_t l_off, float *w,
                                            int lane) {
    using A = typename E::acc_t;
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
    w[lane] = w0;
    w[lane + 64] = w1;
    __syncthreads();
    if (!live) return;

    const float inv = seen ? 1.0f / wsum : 0.0f;
    for (int x = lane; x < a.d; x += 64) {
        float acc = 0.0f;
        if (seen)
            for (int s = 0; s < a.num_splits; ++s) acc += w[s] * a.o_part[((int64_t)s * a.rows + row) * a.d + x];
        E::store(a.O, o_off + (int64_t)x * a.os[3], (A)(acc * inv));
    }
    if (lane == 0) E::store(a.L, l_off, seen ? (A)(m + log2f(wsum)) : (A)INFINITY);
}


template <class E> __global__ __launch_bounds__(kRowsPerBlock * 64) void fa2_decode_combine_kernel(const CombineArgs a) {
    __shared__ float w_lds[kRowsPerBlock][FA2_KVCACHE_MAX_SPLITS];  // the weights of a row, computed once
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (a.cu_q) {  // packed: this block's share of the n_q(b) * H rows of sequence blockIdx.y, row by row as below
        int start, n;
        fa2_varlen_seq(a.cu_q, blockIdx.y, a.total_q, a.max_q, start, n);
        const int64_t own = (int64_t)n * a.H;
        for (int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock; r0 < own; r0 += (int64_t)gridDim.x * kRowsPerBlock) {
            const bool live = r0 + wave < own;
            const int64_t row = (int64_t)start * a.H + (live ? r0 + wave : 0);
            const int64_t tok = row / a.H;
            const int h = (int)(row - tok * a.H);
            combine_row<E>(a, row, live, tok * a.os[2] + h * a.os[1], h * a.ls[1] + tok, w_lds[wave], lane);
        }
        return;
    }
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + wave;
    const bool live = row < a.rows;  // (no early return: one barrier below)
    const int64_t rowc = live ? row : 0;
    const int q = (int)(rowc % a.N_q);
    const int64_t bh = rowc / a.N_q;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    combine_row<E>(a, row, live, b * a.os[0] + h * a.os[1] + (int64_t)q * a.os[2], b * a.ls[0] + h * a.ls[1] + q, w_lds[wave], lane);
}


template <class E> int launch_e(const Fa2DecodeProblem &p, const CombineArgs &a) {
    int64_t nblk = (a.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    if (p.cu_q) {  // per sequence: enough blocks for its longest possible run of rows, at most kPackedBlocks in the whole grid
        nblk = ((int64_t)p.max_q * p.H + kRowsPerBlock - 1) / kRowsPerBlock;
        const int64_t cap = kPackedBlocks / p.B > 1 ? kPackedBlocks / p.B : 1;
        nblk = nblk < cap ? nblk : cap;
    }
    if (nblk > 0x7fffffffLL) {
        fa2_set_error("kvcache combine: grid too large");
        return FA2_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL((fa2_decode_combine_kernel<E>), dim3((unsigned)nblk, p.cu_q ? p.B : 1), dim3(kRowsPerBlock * 64), 0, p.stream, a);
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
    a.H = p.H; a.N_q = p.N_q; a.d = p.d_v; a.num_splits = p.num_splits;
    a.cu_q = p.cu_q; a.total_q = p.total_q; a.max_q = p.max_q;
    if (p.cu_q) a.rows = (int64_t)p.total_q * p.H;
    switch (p.dtype) {
    case FA2_DTYPE_F32: return launch_e<ElemF32>(p, a);
    case FA2_DTYPE_F16: return launch_e<ElemF16>(p, a);
    case FA2_DTYPE_BF16: return launch_e<ElemBF16>(p, a);
    case FA2_DTYPE_F64: return launch_e<ElemF64>(p, a);
    default: fa2_set_error("kvcache: dtype enum %d is not supported", p.dtype); return FA2_ERR_UNSUPPORTED;
    }
}
