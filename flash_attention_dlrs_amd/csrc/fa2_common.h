// Shared declarations of the gfx950 FA-2 forward kernels (internal; the public ABI is include/fa2_fwd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fa2_fwd.h"

// One forward problem, as handed over by fa2_fwd().  Strides in elements (reference convention,
// src/flash_attention_torch.py:53-57).
struct Fa2Problem {
    const void *Q, *K, *V;
    void *O, *L;
    int64_t qs[4], ks[4], vs[4], os[4], ls[2];
    int32_t B, H, N, d;
    int32_t dtype, causal;
    float scale;
    hipStream_t stream;
    int32_t wl, wr;  // local-attention window after fa2_window_normalise(): sides in [0, N-1], N-1 = unbounded (window launchers only)
    // Variable-length (packed) problems (fa2_fwd_varlen, varlen launchers only): B sequences, strides {0, head, token, dim} in
    // qs/ks/vs/os, ls = {0, head stride of L}; wl / wr are the raw sides (-1 = unbounded), causal as given.
    const int32_t *cu_q, *cu_k;
    int32_t max_q, max_k, total_q, total_k;
    int32_t dv;  // fa2_fwd_varlen_dv only: V's and O's last axis (d is Q's and K's); 0 in every other call
};

// Launchers, one per translation unit -- but the six fa2_launch_generic* of fa2_generic.hip and the five fa2_launch_mfma16d* of
// fa2_mfma16d.hip, whose one kernel template takes the attention form as a parameter.  Return FA2_OK / FA2_ERR_*; set_error() on
// failure.
int fa2_launch_generic(const Fa2Problem &p);
int fa2_launch_mfma16(const Fa2Problem &p, int waves);
int fa2_launch_mfma32(const Fa2Problem &p);
int fa2_launch_mfma16d(const Fa2Problem &p, int waves);
int fa2_launch_mfma8x(const Fa2Problem &p, int waves);
int fa2_launch_mfma16k(const Fa2Problem &p, int shape);
#ifdef FA2_EXPERIMENTS   // libfa2_hip_exp.so only (fa2_experiments.h)
#include "fa2_experiments.h"
int fa2_launch_mfma16p(const Fa2Problem &p, int waves, int opt);
int fa2_launch_mfma16x(const Fa2Problem &p, int abl);
int fa2_launch_mfma8(const Fa2Problem &p, int waves);
int fa2_launch_mfma16s(const Fa2Problem &p, int waves);
#endif
int fa2_launch_mfma16h(const Fa2Problem &p, int waves);  // dispatches to the two translation units below
int fa2_launch_mfma16h_causal(const Fa2Problem &p, int waves);
int fa2_launch_mfma16h_noncausal(const Fa2Problem &p, int waves);
// Local attention (fa2_fwd_window).
int fa2_launch_generic_window(const Fa2Problem &p);
int fa2_launch_mfma16d_window(const Fa2Problem &p, int waves);
// Variable-length attention (fa2_fwd_varlen).
int fa2_launch_generic_varlen(const Fa2Problem &p);
int fa2_launch_mfma16d_varlen(const Fa2Problem &p, int waves);
// Grouped-query attention (fa2_fwd_gqa, fa2_fwd_varlen_gqa): K and V have p.H / gqa heads, query head h reads KV head h / gqa.  The
// windowed GQA forms take the dense layouts the host remap cannot merge (a plain or causal problem as the full band).
int fa2_launch_generic_window_gqa(const Fa2Problem &p, int gqa);
int fa2_launch_mfma16d_window_gqa(const Fa2Problem &p, int waves, int gqa);
int fa2_launch_generic_varlen_gqa(const Fa2Problem &p, int gqa);
int fa2_launch_mfma16d_varlen_gqa(const Fa2Problem &p, int waves, int gqa);
// A value head size of its own (fa2_fwd_varlen_dv): V and O have p.dv columns, the scores run over p.d.  The VALU form is the varlen
// GQA instantiation of fa2_generic.hip with the kDv form bit; the matrix kernel (fa2_mfma16dv.hip) takes d = 192, d_v = 128.
// gqa = 1 without grouped heads.
int fa2_launch_generic_varlen_dv(const Fa2Problem &p, int gqa);
int fa2_launch_mfma16dv(const Fa2Problem &p, int gqa);
bool fa2_mfma16dv_supports(const Fa2Problem &p);
// Validates and normalises a window (include/fa2_fwd.h): FA2_ERR_BAD_ARG for a side < -1.  On FA2_OK *windowed = 0 means the window
// removes nothing beyond what plain (*causal_out = 0) or causal (*causal_out = 1) attention removes; *windowed = 1 means the band
// [i - *wl_out, i + *wr_out] with both sides in [0, N - 1] (N - 1 = unbounded), the causal clamp already applied to *wr_out.
int fa2_window_normalise(int32_t N, int32_t causal, int32_t wl, int32_t wr, int32_t *causal_out, int32_t *wl_out, int32_t *wr_out,
                         int32_t *windowed);
// Grouped-query attention: FA2_ERR_BAD_ARG ("H_kv" in the message) unless 1 <= H_kv and H_kv divides H (H < 1 is validate()'s).
int fa2_check_gqa(int32_t H, int32_t H_kv);
int fa2_launch_a64(const Fa2Problem &p);  // generated assembly kernel (asm/fa2_a64_gen.py)
bool fa2_a64_supports(const Fa2Problem &p);
int fa2_launch_a16(const Fa2Problem &p);  // the same structure on v_mfma_f32_16x16x32 (asm/fa2_a16_gen.py)
bool fa2_a16_supports(const Fa2Problem &p);
int fa2_launch_a8(const Fa2Problem &p);   // ... and on the fp8 matrix path, v_mfma_f32_32x32x64_f8f6f4 (asm/fa2_a8_gen.py)
bool fa2_a8_supports(const Fa2Problem &p);
int fa2_launch_a64d(const Fa2Problem &p); // ... and at head size 64 (asm/fa2_a64d_gen.py)
bool fa2_a64d_supports(const Fa2Problem &p);
bool fa2_mfma8_supports(const Fa2Problem &p);
bool fa2_mfma8x_supports(const Fa2Problem &p);
bool fa2_mfma16_supports(const Fa2Problem &p);
bool fa2_mfma16_supports_dp(const Fa2Problem &p);   // + the other multiples of 8 up to 128 (fa2_mfma16.hip only)
bool fa2_mfma32_supports(const Fa2Problem &p);

void fa2_set_error(const char *fmt, ...);
// Tuning knobs for A/B runs.  The product build returns `dflt` without touching the environment (no getenv on the launch
// path); `make experiments` (-DFA2_TUNING_ENV) reads the variable per call.
int fa2_env_int(const char *name, int dflt);

// Per-DEVICE launch state (a process may drive several GPUs): the CU count of the current device, and a once-per-device
// latch for hipFuncSetAttribute(MaxDynamicSharedMemorySize) -- function attributes are per device.
int fa2_device_cus();
struct Fa2DeviceLatch {
    unsigned long long done = 0;  // bit d: applied on device d (a racing second application is harmless: idempotent)
    bool need() const;            // true if the current device has not been marked yet
    void mark();
};

static inline int fa2_dtype_size(int dt) {
    switch (dt) {
    case FA2_DTYPE_F64: return 8;
    case FA2_DTYPE_F32: return 4;
    case FA2_DTYPE_F16:
    case FA2_DTYPE_BF16: return 2;
    case FA2_DTYPE_F8E5M2:
    case FA2_DTYPE_F8E4M3: return 1;
    default: return 0;
    }
}

#define FA2_LOG2E 1.4426950408889634  // np.log2(np.e), src/flash_attention_kernels.py:9

// The attention forms of the kernel templates that take them as a parameter F (fa2_generic_kernel.h, fa2_bwd_generic.hip,
// fa2_mfma16d_kernel.h): a set of these bits, 0 = plain attention.  kWindow: the band i - wl <= j <= i + wr;
// kVarlen (with kWindow): packed sequences; kGqa (with kWindow): H / gqa KV heads; kDv (VALU kernels, with kVarlen and kGqa): a value
// head size of its own.  What a bit means inside a kernel is described at the head of that kernel's file.
constexpr int kWindow = 1, kVarlen = 2, kGqa = 4, kDv = 8;

// Sequence b of a packed (varlen) batch: every offset read is clamped to [0, total], end < start is empty and at most max_len
// rows are taken -- malformed offsets give wrong numbers at worst, never an access outside the tensors.
__device__ __forceinline__ void fa2_varlen_seq(const int32_t *cu, int b, int total, int max_len, int &start, int &len) {
    int s = cu[b], e = cu[b + 1];
    s = s < 0 ? 0 : (s > total ? total : s);
    e = e < 0 ? 0 : (e > total ? total : e);
    const int n = e - s;
    start = s;
    len = n < 0 ? 0 : (n > max_len ? max_len : n);
}

// The sequence that owns packed row t (0 <= t < total), for the kernels that take one packed row per workgroup (the sparse latent
// call's packed forms, the packed selection of the indexer): the last b in [0, B) whose clamped offset is <= t (sequence 0 when none
// is) by a binary search, at most 16 steps for B <= 65535 -- t is uniform, so every step is a scalar load -- then fa2_varlen_seq of
// that b.  False where b does not own t: a gap between sequences, the surplus of a span past max_len, a row at or past the last
// offset.  Any contents of cu give b in [0, B) and start + len <= total.
__device__ __forceinline__ bool fa2_varlen_owner(const int32_t *cu, int B, int total, int max_len, int t, int &b, int &start, int &len) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        int c = cu[mid];
        c = c < 0 ? 0 : (c > total ? total : c);
        if (c <= t) lo = mid;
        else hi = mid;
    }
    b = lo;
    fa2_varlen_seq(cu, b, total, max_len, start, len);
    return t >= start && t - start < len;
}

// The band of a packed sequence of nq queries and nk keys in the windowed kernels' terms -- key j visible to query i iff
// i - wl <= j <= i + wr -- from the raw sides (-1 unbounded; causal clamps the right side to 0), bottom-right aligned: both are
// shifted by nk - nq.  Either side may come out negative.  |wl|, |wr| <= 2 nq + nk (max_seqlen <= 2^28 keeps i + wr in int).
__device__ __forceinline__ void fa2_varlen_band(int nq, int nk, int causal, int wl_raw, int wr_raw, int &wl, int &wr) {
    const int full = nq + nk;  // a side this wide removes nothing
    const int l = (wl_raw < 0 || wl_raw > full) ? full : wl_raw;
    const int r = causal ? 0 : ((wr_raw < 0 || wr_raw > full) ? full : wr_raw);
    wl = l - (nk - nq);
    wr = r + (nk - nq);
}
