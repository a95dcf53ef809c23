// fa2_api.hip -- extern "C" entry points of libfa2_hip.so (declared in include/fa2_fwd.h) and the
// static gfx950 tile table that stands in for the reference's run-time autotuner
// (src/autotune_configs.py:24-201, src/flash_attention_kernels.py:11-15: 114 Triton configs,
// pruned by an SRAM heuristic and benchmarked on first use of every (B, H, N, d)).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fa2_host.h"

namespace {
thread_local char g_err[512] = "";

int validate(const Fa2Problem &p) {
    if (!p.Q || !p.K || !p.V || !p.O || !p.L) {
        fa2_set_error("null tensor pointer");
        return FA2_ERR_BAD_ARG;
    }
    if (p.B <= 0 || p.H <= 0 || p.d <= 0) {
        fa2_set_error("B, H, d must be positive (got B=%d H=%d d=%d)", p.B, p.H, p.d);
        return FA2_ERR_BAD_ARG;
    }
    if (p.N < 1) {
        fa2_set_error("N must be >= 1 (got %d)", p.N);
        return FA2_ERR_BAD_N;
    }
    if (fa2_dtype_size(p.dtype) == 0) {
        fa2_set_error("unknown dtype enum %d", p.dtype);
        return FA2_ERR_UNSUPPORTED;
    }
    // The reference's host glue pads d to max(next_pow2(d), 16) before launching (src/flash_attention_torch.py:38); here
    // any head size goes to the kernels as it is: the MFMA kernels zero-fill the missing columns
    // on load, the generic kernel loops to d.
    if (p.d < 1 || p.d > 512) {
        fa2_set_error("d=%d must be in [1, 512]", p.d);
        return FA2_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < 4; ++k)
        if (p.qs[k] < 0 || p.ks[k] < 0 || p.vs[k] < 0 || p.os[k] < 0) {
            fa2_set_error("negative strides are not supported");
            return FA2_ERR_BAD_ARG;
        }
    if (p.os[3] == 0 || (p.N > 1 && p.os[2] == 0)) {
        fa2_set_error("O must not alias itself (zero stride)");
        return FA2_ERR_BAD_ARG;
    }
    if (!(p.scale == p.scale)) {
        fa2_set_error("scale is NaN");
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

// The thresholds of the tables below were measured on the full chip (256 CUs) and are written in tiles / jobs per 256 CUs: T(n) scales
// them to the CU count of the current device (a partitioned or smaller part fills at proportionally smaller grids).
struct Tiles {
    const int cus = fa2_device_cus();
    long long operator()(long long n) const { return (n * cus + 128) / 256; }
};

// n rows (and 512 of overrun) of K and V -- and of O, unless the problem is packed -- stay below the 2 GiB of a 32-bit buffer offset
bool fits32(const Fa2Problem &p, int64_t n) {
    const auto fits = [n](int64_t row) { return (n + 512) * row * 2 < (1LL << 31); };
    return fits(p.ks[2]) && fits(p.vs[2]) && (p.cu_q || fits(p.os[2]));
}

long long tiles256(const Fa2Problem &p) { return (long long)((p.N + 255) / 256) * p.B * p.H; }

// The jobs of a persistent grid of one 8-wave workgroup per CU (256-row tiles, tile PAIRS when causal), and whether they fill
// `cus` CUs evenly: its time goes in steps of whole jobs per CU, and at most 20 % may be lost to them.
long long jobs256(const Fa2Problem &p) {
    const int nq256 = (p.N + 255) / 256;
    return (long long)(p.causal ? (nq256 + 1) / 2 : nq256) * p.B * p.H;
}
bool even(long long jobs, int cus) {
    const double x = (double)jobs / (double)cus;
    return x <= 1.0 ? x >= 0.6 : (double)((jobs + cus - 1) / cus) / x <= 1.2;
}

// The static tile table, keyed like the reference's autotuner on (B, H, N, d) (plus dtype, causal, strides): the grid
// size B * H * tiles decides between the key-split, 4-wave and one-workgroup-per-CU kernels.
int pick_variant(const Fa2Problem &p) {
    const Tiles T;
    if (fa2_mfma16_supports(p)) {
        // Software-pipelined kernel with LDS-DMA staging.  8 waves x 32 rows halves the K/V traffic per query
        // row; it needs enough 256-row tiles to fill 256 CUs, otherwise the 128-row tile spreads the work wider.
        // (N * row stride >= 2 GiB does not fit the 32-bit buffer offsets: fall back to the first MFMA kernel.)
        const long long wg256 = tiles256(p);
        if (!fits32(p, p.N)) return wg256 >= T(512) ? FA2_VARIANT_MFMA16_W8 : FA2_VARIANT_MFMA16;
        // d = 128, N a multiple of 256: the generated assembly kernel A64 (4 waves x 64 rows, one wave per SIMD, O / Q / V^T in
        // the accumulator file) wins from 64 jobs of 256 rows on -- a quarter of the CUs busy -- non-causal, and causal from
        // 192 jobs (or 96 when a job has at least eight key tiles); below that the key-split kernels keep more CUs busy.
        // benchmarks/mid_grid.py, 48 shapes, bf16, d = 128, profiles/r02/mid_grid_a64.jsonl: against the best of
        // MFMA16D_W4 / MFMA16H / MFMA16K it is 4-33 % faster on every shape from those sizes up (the persistent grid also
        // takes job counts that are not a multiple of the CU count better: 1.5 jobs per CU 180 vs 213 us); on the same
        // MI355X against MFMA16H: c3 causal +15-19 %, c3 shape non-causal +15-17 %.
        // head size 64: the generated kernel at d = 64 (A64D, asm/fa2_a64d_gen.py; N a multiple of 256 or its ragged form) under a64's grid rule.
        // Same-device A/B against the rest of this table (profiles/r03/a64d_vs_table.jsonl), bf16 / f16: B8 H16 N4096 1 013 vs 840
        // TFLOP/s (+21 %), causal 1 014 vs 827 (+23 %); N = 8192 1 092 vs 929, causal 1 060 vs 887; B16 H32 N2048 984 vs 821,
        // causal 860 vs 677 (+27 %)
        // Grid rule from the d = 64 mid-grid sweep (benchmarks/mid_grid.py, profiles/r03/mid_grid_d64.jsonl, 48 shapes): from 192 jobs
        // of 256 rows on A64D is the best of the six kernels or within 4 % of it; below, the key-split and 128-row kernels keep more
        // CUs busy (64 jobs: 13.1 us for MFMA16K_R2K4 against 17.0)
        // (f16 at the reference's scale of 1 -- rescales every few tiles, see A64 below -- causal: only from 384 jobs = 192 units on;
        // at 128 units the 8-wave kernels lead by 3 .. 13 %, profiles/r03/mid_grid_f16_d64.jsonl)
        const bool f16_hot = p.dtype == FA2_DTYPE_F16 && p.scale > 0.5f;
        if (fa2_a64d_supports(p) && wg256 >= T(p.causal ? (f16_hot ? 384 : 192) : 160)) return FA2_VARIANT_A64D;
        // f16 at the reference's scale of 1 rescales every few tiles (P must stay below 65 504); with one wave per SIMD a rescale is
        // ~2 000 cycles with three waves waiting, which the 8-wave kernels hide.  On a full chip A64 still leads; on half-filled
        // grids it loses 12 .. 30 % to them (profiles/r03/mid_grid_f16.jsonl: 64 jobs 30.9 vs 21.5 us, 128 jobs 32.0 vs 27.0, causal
        // N = 2048 128 jobs 60.1 vs 45.2), where bf16 -- which never rescales -- wins.  At softmax scales <= 0.5 f16 behaves like bf16.
        const bool a64_grid = f16_hot ? wg256 >= T(256)
                                      : (p.causal ? (wg256 >= T(192) || (wg256 >= T(96) && p.N >= 2048)) : wg256 >= T(64));
        if (fa2_a64_supports(p) && a64_grid) {
            // The same kernel on the other matrix shape (A16: v_mfma_f32_16x16x32, asm/fa2_a16_gen.py): 15 % more cycles per key
            // step, but the chip holds a 10-17 % higher clock under it.  Same-device A/B against A64 (benchmarks/variants.py,
            // profiles/r03/a16_vs_a64.jsonl), bf16: non-causal N = 4096 +2.4 .. +4.4 %, N = 8192 (BASELINE configs[3]'s shard)
            // +4.4 %, N = 2048 +1.3 %; causal N = 8192 +2.0 %, N = 4096 -1.0 %, N = 2048 -3.5 % (short jobs: the seam and the
            // epilogue grow with the cycles, the clock gain is smaller there); f16 (rescales every few tiles) -2.5 %.
            // f16 at the reference's scale of 1 rescales every few tiles (P must stay below 65 504), which the 16x16 form pays for
            // twice (-3 %); at the usual softmax scales the maximum rarely moves: scale 0.5 / 0.25 / 1 / sqrt(128) on the reference
            // bench's shape: +3.0 / +5.4 / +3.6 % (scripts/gpu_f16_scale.sh, profiles/r03/f16_scale_a16_vs_a64.jsonl)
            const bool a16_dtype = p.dtype == FA2_DTYPE_BF16 || (p.dtype == FA2_DTYPE_F16 && p.scale <= 0.5f);
            // ... and only where the chip is full enough to sit on its power limit: on half-filled grids (128 jobs, or 128 causal
            // units: 2.4 GHz whatever the shape) the extra cycles cost 15 % (profiles/r03/mid_grid_final.jsonl: N = 4096 B*H = 8 78.9 vs
            // 68.3 us, causal N = 8192 B*H = 8 158.2 vs 137.8); from 192 jobs on it leads
            const long long units16 = p.causal ? (wg256 + 1) / 2 : wg256;
            if (a16_dtype && (p.causal ? p.N >= 8192 : p.N >= 4096) && units16 >= T(192)) return FA2_VARIANT_A16;
            return FA2_VARIANT_A64;
        }
        // Small grids: at most 128 work units (128-row tiles, tile PAIRS when causal) leave half of the 256 CUs idle and
        // every workgroup walks its key tiles in sequence -- latency-bound.  MFMA16K splits the keys of a tile among
        // wave groups of the same workgroup (no workspace): benchmarks/tiny_grid.py, HIP-graph replay, fp16:
        // B2 H8 N1024 d64 (BASELINE.json configs[1]) 16.8 -> 11.2 us; d = 128 25.3 -> 21.2; causal d = 128 38.6 -> 21.2;
        // B1 H8 N4096 d128 causal 112.8 -> 79.3.  At 192 units and above the plain kernels are as fast or faster.
        const long long wg128 = (long long)((p.N + 127) / 128) * p.B * p.H;
        if ((p.causal ? wg128 / 2 : wg128) <= T(128)) {
            // causal, 129..256 tiles: 128-row tiles, two key groups -- except d = 64 at two 64-row workgroups per CU and long rows,
            // where the (2, 4) shape leads (mid_grid_final.jsonl: N = 4096 B*H = 8 39.6 vs 51.2 us, N = 2048 B*H = 16 25.0 vs 29.1; at
            // 1.5 per CU or N = 1024 it loses)
            if (wg128 > T(128)) return p.d == 64 && p.N >= 2048 && wg128 > T(224) ? FA2_VARIANT_MFMA16K_R2K4 : FA2_VARIANT_MFMA16K;
            if (p.d == 64 && p.N >= 512) return FA2_VARIANT_MFMA16K_R2K4;
            return FA2_VARIANT_MFMA16K_R2K2;
        }
        // Mid-size grids (benchmarks/mid_grid.py, profiles/r01/mid_grid_bf16.jsonl: 96 shapes, bf16, 64..1024 256-row
        // tiles).  MFMA16H is a persistent grid of one 8-wave workgroup per CU: its time goes in steps of whole jobs per
        // CU (256-row tiles, tile PAIRS when causal), so it wants the job count near a multiple of 256; the 4-wave
        // MFMA16D_W4 has twice the jobs at half the size.  Readings behind the rules: d = 128 non-causal, 192 / 256 tiles:
        // MFMA16H -12..16 % / -5..10 %, 384 tiles (1.5 jobs per CU): MFMA16D_W4 -5 %; d = 128 causal, 384 tiles: MFMA16H
        // -16..19 %; d = 64 causal, 768 tiles (1.5 pairs per CU): MFMA16D_W4
        // -20 %, 256 tiles: MFMA16D_W4 -25 %.
        const bool even_h = even(jobs256(p), T.cus);  // MFMA16H's jobs: <= 20 % lost to whole jobs
        // (two full rounds of the 8-wave key-split workgroups: B1 H16 N4096 98 vs 105 us, B1 H8 N8192 173 vs 191; at
        // 1.5 rounds -- 384 tiles -- it loses 50 %)
        if (p.causal && p.d == 128 && wg128 > T(448) && wg128 <= T(512) && p.N >= 4096) return FA2_VARIANT_MFMA16K;
        if (p.d == 128) {
            if (p.causal ? wg256 < T(320) : (wg256 < T(160) || !even_h)) return FA2_VARIANT_MFMA16D_W4;
        } else {
            if (wg256 < T(160) || !even_h) return FA2_VARIANT_MFMA16D_W4;
        }
        // 8-wave tiles: MFMA16H (persistent grid, next-job prefetch, hand-ordered steady loop).  Against MFMA16D on
        // MI355X (benchmarks/lottery.py, alternating order): non-causal +4.4 % (d = 128, N = 4096), +3.4 % (N = 8192),
        // +9 % (d = 64); causal, once its causal kernels got a translation unit of their own: +4.1 % at the north-star
        // shape (N = 4096), +4 % (N = 2048), +2.6 % (N = 8192), +2.5 % (N = 16384), +2.4 % (d = 64).
        return FA2_VARIANT_MFMA16H;
    }
    // (The generated fp8 kernel A8 -- asm/fa2_a8_gen.py: the A64 structure on v_mfma_f32_32x32x64_f8f6f4 -- in its first form rescaled
    // O whenever the running maximum moved, like MFMA8X: with one wave per SIMD that cost ~900 cycles per rescale with three waves
    // waiting, and on N(0, 1) inputs (scores of sigma 16 log2 units against fp8's few units of deferral) it lost to the 8-wave kernel,
    // 2 080 vs 2 216 TFLOP/s on BASELINE configs[4]'s shard.  Its P.V now runs on the BLOCK-SCALED MFMA: the running maximum is an
    // integer and the power of two rides in P's E8M0 scale operand, O is never touched: 2 457 vs 2 260 on N(0, 1), 2 418 vs 2 231 on
    // N(0, 1/4) (profiles/r03/a8_scaled_vs_mfma8x.jsonl); grids: benchmarks/mid_grid_fp8.py, profiles/r03/mid_grid_fp8_a8.jsonl)
    if (fa2_mfma8x_supports(p)) {
        // fp8: the double-rate k = 64 MFMA (64-key units).  Against MFMA8 (32x32x16 fp8, the bf16 rate) on MI355X:
        // +26 % at the c5 per-GPU shape (N = 16384 non-causal: 1 880 vs 1 492 TFLOP/s), +19 % at c3 causal.
        // 8 waves (one workgroup per CU) when the job count -- 256-row tiles, tile pairs when causal -- fills the 256 CUs
        // evenly, else 4 waves: the rule of the bf16 table above, checked on 52 fp8 shapes (benchmarks/mid_grid_fp8.py,
        // profiles/r01/mid_grid_fp8.jsonl; the old single threshold lost up to 20 % at 1.5 jobs per CU).
        const long long wg256 = tiles256(p);
        const bool even_x = even(jobs256(p), T.cus);
        // the generated kernel (N a multiple of 256): best or equal on every even grid from 192 jobs on, +5 .. +9 % from 512 jobs on
        // (causal: +8 .. +19 %, profiles/r03/mid_grid_fp8_a8_causal.jsonl, a8_causal_vs_mfma8x.jsonl); at 1.5 jobs per CU (384) its
        // whole-job steps lose 10 % to the 4-wave kernel like the 8-wave one's
        if (fa2_a8_supports(p) && wg256 >= T(192) && even_x) return FA2_VARIANT_A8;
        return wg256 >= T(160) && even_x ? FA2_VARIANT_MFMA8X : FA2_VARIANT_MFMA8X_W4;
    }
    if (fa2_mfma32_supports(p)) return FA2_VARIANT_MFMA32;
    // 16-bit head sizes other than 64 / 128 (multiples of 8): the first MFMA kernel with the missing columns zero-filled
    // on load; 8 waves when there are enough 256-row tiles for the 256 CUs
    if (fa2_mfma16_supports_dp(p))
        return tiles256(p) >= T(512) ? FA2_VARIANT_MFMA16_W8 : FA2_VARIANT_MFMA16;
    return FA2_VARIANT_GENERIC;
}

// The dense table: every variant id with its launcher and its tile (B_r, B_c, waves), which fa2_query_tile_scaled reports.  The
// experimental kernels, their A/B schedules and the timing-only ablations (wrong results by construction) are rows of the
// experiments and ablation builds only.
using P = const Fa2Problem &;
struct DenseRow {
    int id;
    int (*launch)(P);
    int B_r, B_c, waves;
};
const DenseRow kDense[] = {
    {FA2_VARIANT_GENERIC, fa2_launch_generic, 16, 64, 4},
    {FA2_VARIANT_MFMA16, [](P p) { return fa2_launch_mfma16(p, 4); }, 128, 64, 4},
    {FA2_VARIANT_MFMA16_W8, [](P p) { return fa2_launch_mfma16(p, 8); }, 256, 64, 8},
    {FA2_VARIANT_MFMA32, fa2_launch_mfma32, 128, 32, 4},
    {FA2_VARIANT_MFMA8X, [](P p) { return fa2_launch_mfma8x(p, 8); }, 256, 64, 8},
    {FA2_VARIANT_MFMA8X_W4, [](P p) { return fa2_launch_mfma8x(p, 4); }, 128, 64, 4},
    {FA2_VARIANT_MFMA16K, [](P p) { return fa2_launch_mfma16k(p, 42); }, 128, 64, 8},
    {FA2_VARIANT_MFMA16K_R2K2, [](P p) { return fa2_launch_mfma16k(p, 22); }, 64, 64, 4},
    {FA2_VARIANT_MFMA16K_R2K4, [](P p) { return fa2_launch_mfma16k(p, 24); }, 64, 64, 8},
    {FA2_VARIANT_MFMA16D, [](P p) { return fa2_launch_mfma16d(p, 8); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16D_W4, [](P p) { return fa2_launch_mfma16d(p, 4); }, 128, 32, 4},
    {FA2_VARIANT_MFMA16H, [](P p) { return fa2_launch_mfma16h(p, 8); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16H_W4, [](P p) { return fa2_launch_mfma16h(p, 4); }, 128, 32, 4},
    {FA2_VARIANT_A64, fa2_launch_a64, 256, 64, 4},
    {FA2_VARIANT_A16, fa2_launch_a16, 256, 64, 4},
    {FA2_VARIANT_A8, fa2_launch_a8, 256, 64, 4},
    {FA2_VARIANT_A64D, fa2_launch_a64d, 256, 64, 4},
#ifdef FA2_EXPERIMENTS
    {FA2_VARIANT_MFMA16P, [](P p) { return fa2_launch_mfma16p(p, 4, 0); }, 128, 32, 4},
    {FA2_VARIANT_MFMA16P_W8, [](P p) { return fa2_launch_mfma16p(p, 8, 64); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16X, [](P p) { return fa2_launch_mfma16x(p, 0); }, 256, 32, 4},
    {FA2_VARIANT_MFMA8, [](P p) { return fa2_launch_mfma8(p, 8); }, 256, 32, 8},
    {FA2_VARIANT_MFMA8_W4, [](P p) { return fa2_launch_mfma8(p, 4); }, 128, 32, 4},
    {FA2_VARIANT_MFMA8U, [](P p) { return fa2_launch_mfma8x(p, 12); }, 128, 64, 4},
    {FA2_VARIANT_MFMA16S, [](P p) { return fa2_launch_mfma16s(p, 8); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16S_W4, [](P p) { return fa2_launch_mfma16s(p, 4); }, 128, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 1, [](P p) { return fa2_launch_mfma16x(p, 1); }, 256, 32, 4},   // ablations (FA2_ABLATIONS builds)
    {FA2_VARIANT_MFMA16X + 2048 * 3, [](P p) { return fa2_launch_mfma16x(p, 3); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 4, [](P p) { return fa2_launch_mfma16x(p, 4); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 7, [](P p) { return fa2_launch_mfma16x(p, 7); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 8, [](P p) { return fa2_launch_mfma16x(p, 8); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 15, [](P p) { return fa2_launch_mfma16x(p, 15); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 16, [](P p) { return fa2_launch_mfma16x(p, 16); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 32, [](P p) { return fa2_launch_mfma16x(p, 32); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16X + 2048 * 48, [](P p) { return fa2_launch_mfma16x(p, 48); }, 256, 32, 4},
    {FA2_VARIANT_MFMA16P + 16, [](P p) { return fa2_launch_mfma16p(p, 4, 1); }, 128, 32, 4},     // experimental schedules (A/B only)
    {FA2_VARIANT_MFMA16P_W8 + 16, [](P p) { return fa2_launch_mfma16p(p, 8, 1); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 32, [](P p) { return fa2_launch_mfma16p(p, 8, 2); }, 256, 32, 8},   // ablations: only in -DFA2_ABLATIONS builds
    {FA2_VARIANT_MFMA16P_W8 + 64, [](P p) { return fa2_launch_mfma16p(p, 8, 4); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 128, [](P p) { return fa2_launch_mfma16p(p, 8, 8); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 224, [](P p) { return fa2_launch_mfma16p(p, 8, 14); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 256, [](P p) { return fa2_launch_mfma16p(p, 8, 16); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 512, [](P p) { return fa2_launch_mfma16p(p, 8, 32); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 736, [](P p) { return fa2_launch_mfma16p(p, 8, 46); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 192 * 16, [](P p) { return fa2_launch_mfma16p(p, 8, 192); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P_W8 + 1024, [](P p) { return fa2_launch_mfma16p(p, 8, 0); }, 256, 32, 8},
    {FA2_VARIANT_MFMA16P + 1024, [](P p) { return fa2_launch_mfma16p(p, 4, 64); }, 128, 32, 4},
#endif
};
const DenseRow *dense_row(int id) {
    for (const DenseRow &row : kDense)
        if (row.id == id) return &row;
    return nullptr;
}

// Windowed table (fa2_fwd_window): the pipelined LDS-DMA kernel where it runs -- 8 or 4 waves by grid fill, rule (3) of the static
// table above -- else the VALU kernel.  The window makes the work per tile uniform away from the sequence ends, so one 128- or
// 256-row tile per workgroup.
int pick_window_variant(const Fa2Problem &p) {
    const Tiles T;
    if (!fa2_mfma16_supports(p) || !fits32(p, p.N)) return FA2_VARIANT_GENERIC;
    return tiles256(p) >= T(160) ? FA2_VARIANT_MFMA16D : FA2_VARIANT_MFMA16D_W4;
}

// Varlen table: the windowed one's kernels, the 32-bit offsets judged on one sequence (max_seqlen_k x row stride, not the packed
// total).  4 waves: one 128-row tile per workgroup measured faster than the 8-wave form on every packed shape benchmarked
// (profiles/varlen/bench_varlen.jsonl; the varlen form has no causal tile pairs to fill a 256-row workgroup)
int pick_varlen_variant(const Fa2Problem &p) {
    return fa2_mfma16_supports(p) && fits32(p, p.max_k) ? FA2_VARIANT_MFMA16D_W4 : FA2_VARIANT_GENERIC;
}

// The table of the other four forms (FA2_FORM_WINDOW .. FA2_FORM_VARLEN_GQA): each takes GENERIC, MFMA16D and MFMA16D_W4 and
// refuses any other id with its own sentence.
struct FormRow {
    int (*generic)(P, int g);
    int (*mfma16d)(P, int waves, int g);
    const char *other;
};
const FormRow kForms[4] = {
    {[](P p, int) { return fa2_launch_generic_window(p); }, [](P p, int waves, int) { return fa2_launch_mfma16d_window(p, waves); },
     "kernel variant %d does not take a window (generic, mfma16d and mfma16d_w4 do)"},
    {[](P p, int) { return fa2_launch_generic_varlen(p); }, [](P p, int waves, int) { return fa2_launch_mfma16d_varlen(p, waves); },
     "kernel variant %d has no varlen form (generic, mfma16d and mfma16d_w4 do)"},
    {fa2_launch_generic_window_gqa, fa2_launch_mfma16d_window_gqa,
     "kernel variant %d has no GQA form for this layout (generic, mfma16d and mfma16d_w4 do; a layout with batch strides H x the head "
     "strides takes every variant)"},
    {fa2_launch_generic_varlen_gqa, fa2_launch_mfma16d_varlen_gqa,
     "kernel variant %d has no varlen GQA form (generic, mfma16d and mfma16d_w4 do)"},
};

// Step 3: the launch of a checked problem in its form, AUTO resolved by the form's table.
int run_fwd(const Fa2Problem &p, Fa2Form form, int variant) {
    if (form.kind == FA2_FORM_DENSE) {
        const DenseRow *row = dense_row(variant == FA2_VARIANT_AUTO ? pick_variant(p) : variant);
        if (row) return row->launch(p);
        fa2_set_error("unknown kernel variant %d", variant);
        return FA2_ERR_BAD_ARG;
    }
    const bool packed = form.kind == FA2_FORM_VARLEN || form.kind == FA2_FORM_VARLEN_GQA;
    if (variant == FA2_VARIANT_AUTO) variant = packed ? pick_varlen_variant(p) : pick_window_variant(p);
    const FormRow &row = kForms[form.kind - FA2_FORM_WINDOW];
    switch (variant) {
    case FA2_VARIANT_GENERIC: return row.generic(p, form.g);
    case FA2_VARIANT_MFMA16D: return row.mfma16d(p, 8, form.g);
    case FA2_VARIANT_MFMA16D_W4: return row.mfma16d(p, 4, form.g);
    default: fa2_set_error(row.other, variant); return FA2_ERR_UNSUPPORTED;
    }
}

// fa2_fwd_varlen_dv: a checked packed problem with a value head size of its own (p.dv).  The matrix kernel where it runs (d 192 /
// d_v 128, 16-bit), else the VALU form; at d_v == d AUTO is the varlen table itself and GENERIC the varlen (GQA) kernel itself, so
// the bits are fa2_fwd_varlen_gqa_variant's.
int run_fwd_dv(const Fa2Problem &p, Fa2Form form, int variant) {
    if (variant == FA2_VARIANT_AUTO) {
        if (p.dv == p.d) return run_fwd(p, form, FA2_VARIANT_AUTO);
        variant = fa2_mfma16dv_supports(p) ? FA2_VARIANT_MFMA16DV : FA2_VARIANT_GENERIC;
    }
    switch (variant) {
    case FA2_VARIANT_GENERIC: return p.dv == p.d ? run_fwd(p, form, FA2_VARIANT_GENERIC) : fa2_launch_generic_varlen_dv(p, form.g);
    case FA2_VARIANT_MFMA16DV: return fa2_launch_mfma16dv(p, form.g);
    default:
        fa2_set_error("kernel variant %d is not one of fa2_fwd_varlen_dv's (generic and mfma16dv are)", variant);
        return FA2_ERR_UNSUPPORTED;
    }
}
}  // namespace

int fa2_launch_mfma16h(const Fa2Problem &p, int waves) {
    return p.causal ? fa2_launch_mfma16h_causal(p, waves) : fa2_launch_mfma16h_noncausal(p, waves);
}

void fa2_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int fa2_env_int(const char *name, int dflt) {
#ifdef FA2_TUNING_ENV
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

namespace {
int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    return dev;
}
}  // namespace

int fa2_device_cus() {
    static int cus[64] = {0};
    const int dev = current_device();
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

bool Fa2DeviceLatch::need() const { return !((__atomic_load_n(&done, __ATOMIC_RELAXED) >> current_device()) & 1ull); }
void Fa2DeviceLatch::mark() { __atomic_fetch_or(&done, 1ull << current_device(), __ATOMIC_RELAXED); }

int fa2_window_normalise(int32_t N, int32_t causal, int32_t wl, int32_t wr, int32_t *causal_out, int32_t *wl_out, int32_t *wr_out,
                         int32_t *windowed) {
    const int rc = fa2_check_window_sides(wl, wr);
    if (rc != FA2_OK) return rc;
    const int32_t full = N > 1 ? N - 1 : 0;  // a side of N - 1 or more removes nothing
    int32_t l = (wl < 0 || wl >= full) ? full : wl, r = (wr < 0 || wr >= full) ? full : wr;
    if (causal) r = 0;
    *causal_out = causal ? 1 : 0;
    *wl_out = l;
    *wr_out = r;
    *windowed = 0;
    if (l == full && r == full) return FA2_OK;  // plain (or N = 1)
    if (l == full && r == 0) {                  // causal
        *causal_out = 1;
        return FA2_OK;
    }
    *windowed = 1;
    return FA2_OK;
}

// H_kv must divide H (fa2_fwd_gqa / fa2_fwd_varlen_gqa and their backward twins): FA2_ERR_BAD_ARG before any launch.
int fa2_check_gqa(int32_t H, int32_t H_kv) {
    if (H_kv < 1) {
        fa2_set_error("H_kv must be >= 1 (got H_kv=%d)", H_kv);
        return FA2_ERR_BAD_ARG;
    }
    if (H >= 1 && H % H_kv != 0) {
        fa2_set_error("H_kv must divide H (got H=%d, H_kv=%d)", H, H_kv);
        return FA2_ERR_BAD_ARG;
    }
    return FA2_OK;
}

namespace {
// Step 1: the raw arguments of any of the twelve forward entry points.  A dense call has 4-element strides {batch, head, token, d}, L's
// two and N; a packed one 3-element strides {token, head, d} and the parts behind `packed`.  Window sides of (-1, -1) are no window.
struct FwdCall {
    const void *Q, *K, *V;
    void *O, *L;
    const int64_t *q_strides, *k_strides, *v_strides, *o_strides, *l_strides;
    int32_t B, H, N, d, dtype_enum, causal;
    float scale;
    void *hip_stream;
    int32_t variant;
    int32_t window_left = -1, window_right = -1;
    bool gqa = false;  // fa2_fwd_gqa, fa2_fwd_varlen_gqa: K and V have H_kv heads
    int32_t H_kv = 0;
    bool packed = false;  // fa2_fwd_varlen, fa2_fwd_varlen_gqa: B sequences over cu_seqlens_*, L is (H, total_q)
    const int32_t *cu_seqlens_q = nullptr, *cu_seqlens_k = nullptr;
    int32_t max_seqlen_q = 0, max_seqlen_k = 0, total_q = 0, total_k = 0;
    int64_t l_head_stride = 0;
    bool has_dv = false;  // fa2_fwd_varlen_dv (a packed GQA call): V and O have d_v columns
    int32_t d_v = 0;
};

// Step 2: every argument tested, in the one order tests/golden/train_host_calls.json records -- H_kv, then a packed call's pointers
// and sizes or a dense call's window, then validate() -- yielding the problem to launch and the form that runs it.
//
// Dense grouped-query attention (H_kv < H).  A mergeable layout -- B == 1, or the batch strides of Q, O, L a multiple H of their
// head strides and those of K, V a multiple H_kv -- is the MHA problem of B' = B * H_kv batches of g = H / H_kv heads each sharing
// one K / V head (head stride 0): every kernel of the dense and windowed tables runs it unchanged, and the table sees the same
// B * H.  Any other layout runs the windowed GQA forms, a plain or causal problem as the full band.
int check_fwd(const FwdCall &c, Fa2Problem &p, Fa2Form &form) {
    form = {FA2_FORM_DENSE, 1};
    if (c.gqa) {  // H_kv must divide H: FA2_ERR_BAD_ARG before anything else
        const int rc = fa2_check_gqa(c.H, c.H_kv);
        if (rc != FA2_OK) return rc;
        if (c.H >= 1) form.g = c.H / c.H_kv;
    }
    memset(&p, 0, sizeof(p));
    p.Q = c.Q; p.K = c.K; p.V = c.V; p.O = c.O; p.L = c.L;
    p.B = c.B; p.H = c.H; p.d = c.d; p.dtype = c.dtype_enum; p.causal = c.causal ? 1 : 0; p.scale = c.scale;
    p.stream = (hipStream_t)c.hip_stream;
    if (c.packed) {
        const void *ptrs[9] = {c.Q, c.K, c.V, c.O, c.L, c.q_strides, c.k_strides, c.v_strides, c.o_strides};
        const char *names[9] = {"Q", "K", "V", "O", "L", "q_strides", "k_strides", "v_strides", "o_strides"};
        int rc = fa2_check_nonnull("varlen", ptrs, names, 9);
        if (rc == FA2_OK) rc = fa2_check_packed("varlen", c, true);
        if (rc != FA2_OK) return rc;
        if (c.dtype_enum == FA2_DTYPE_F8E5M2 || c.dtype_enum == FA2_DTYPE_F8E4M3) {
            fa2_set_error("varlen: fp8 is not supported (no backward; e4m3fn cannot hold L = +inf)");
            return FA2_ERR_UNSUPPORTED;
        }
        fa2_packed_strides4(c.q_strides, p.qs); fa2_packed_strides4(c.k_strides, p.ks);
        fa2_packed_strides4(c.v_strides, p.vs); fa2_packed_strides4(c.o_strides, p.os);
        fa2_set_packed(c, p);
        rc = validate(p);
        if (rc != FA2_OK) return rc;
        if (c.l_head_stride < 0) {
            fa2_set_error("varlen: negative L head stride");
            return FA2_ERR_BAD_ARG;
        }
        if (c.has_dv) {  // (after every check of fa2_fwd_varlen_gqa)
            if (c.d_v < 1 || c.d_v > 512) {
                fa2_set_error("varlen: d_v=%d must be in [1, 512]", c.d_v);
                return FA2_ERR_BAD_ARG;
            }
            p.dv = c.d_v;
        }
        form.kind = form.g > 1 ? FA2_FORM_VARLEN_GQA : FA2_FORM_VARLEN;
        return FA2_OK;
    }
    Fa2Window w;
    int rc = fa2_window_of(c.N, c.causal, c.window_left, c.window_right, w);
    if (rc != FA2_OK) return rc;
    if (c.q_strides && c.k_strides && c.v_strides && c.o_strides && c.l_strides) {
        for (int k = 0; k < 4; ++k) { p.qs[k] = c.q_strides[k]; p.ks[k] = c.k_strides[k]; p.vs[k] = c.v_strides[k]; p.os[k] = c.o_strides[k]; }
        p.ls[0] = c.l_strides[0]; p.ls[1] = c.l_strides[1];
    } else {
        p.Q = nullptr;  // fails validate()
    }
    p.N = c.N;
    p.causal = w.causal;
    rc = validate(p);
    if (rc != FA2_OK) return rc;
    if (w.windowed) {  // (a window that removes nothing beyond plain / causal attention stays the dense form)
        form.kind = FA2_FORM_WINDOW;
        p.causal = 0;
        p.wl = w.wl;
        p.wr = w.wr;
    }
    if (form.g == 1) return FA2_OK;
    const int g = form.g, H_kv = c.H_kv;
    if (H_kv == 1) {  // (a size-1 head dimension may carry any stride -- torch leaves it free: only the batch stride is read)
        p.ks[1] = p.ks[0];
        p.vs[1] = p.vs[0];
    }
    bool mergeable = c.B == 1 || (p.qs[0] == (int64_t)c.H * p.qs[1] && p.os[0] == (int64_t)c.H * p.os[1] &&
                                  p.ls[0] == (int64_t)c.H * p.ls[1] && p.ks[0] == (int64_t)H_kv * p.ks[1] &&
                                  p.vs[0] == (int64_t)H_kv * p.vs[1]);
    if (mergeable && (int64_t)c.B * H_kv > 65535) {
        // the merged problem has B * H_kv batches: the generic kernel's grid takes at most 65535 of them (grid y), so a problem
        // that would run there stays unmerged and runs the GQA form, whose grid holds the B the caller passed
        Fa2Problem m = p;
        m.B = (int64_t)c.B * H_kv > 0x7fffffff ? 0x7fffffff : c.B * H_kv;
        m.H = g;
        const int v = c.variant != FA2_VARIANT_AUTO ? c.variant : (w.windowed ? pick_window_variant(m) : pick_variant(m));
        if (v == FA2_VARIANT_GENERIC || (int64_t)c.B * H_kv > 0x7fffffff) mergeable = false;
    }
    if (mergeable) {
        p.B = c.B * H_kv;  // (<= B * H)
        p.H = g;
        p.qs[0] = g * p.qs[1];
        p.os[0] = g * p.os[1];
        p.ls[0] = g * p.ls[1];
        p.ks[0] = p.ks[1];
        p.ks[1] = 0;
        p.vs[0] = p.vs[1];
        p.vs[1] = 0;
        return FA2_OK;
    }
    form.kind = FA2_FORM_WINDOW_GQA;
    p.causal = 0;  // the band carries the mask: (N - 1, N - 1) plain, (N - 1, 0) causal
    p.wl = w.wl;
    p.wr = w.wr;
    return FA2_OK;
}

int fwd(const FwdCall &c) {
    Fa2Problem p;
    Fa2Form form;
    const int rc = check_fwd(c, p, form);
    if (rc != FA2_OK) return rc;
    return c.has_dv ? run_fwd_dv(p, form, c.variant) : run_fwd(p, form, c.variant);
}

// What every entry point fills alike (a packed one: 3-element strides, no l_strides, no N); the rest each adds its own.
FwdCall dense_call(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t *qs, const int64_t *ks, const int64_t *vs,
                   const int64_t *os, const int64_t *ls, int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal,
                   float scale, void *hip_stream, int32_t variant) {
    FwdCall c;
    c.Q = Q; c.K = K; c.V = V; c.O = O; c.L = L; c.q_strides = qs; c.k_strides = ks; c.v_strides = vs; c.o_strides = os; c.l_strides = ls;
    c.B = B; c.H = H; c.N = N; c.d = d; c.dtype_enum = dtype_enum; c.causal = causal; c.scale = scale; c.hip_stream = hip_stream;
    c.variant = variant;
    return c;
}
}  // namespace

// Every entry point fills a call and hands it to fwd(); X is X_variant with FA2_VARIANT_AUTO.
extern "C" {

int fa2_fwd(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
            const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
            const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
            int32_t causal, float scale, void *hip_stream) {
    return fa2_fwd_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, B, H, N, d, dtype_enum, causal, scale,
                           hip_stream, FA2_VARIANT_AUTO);
}

int fa2_fwd_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                    const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                    const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
                    int32_t causal, float scale, void *hip_stream, int32_t variant) {
    return fwd(dense_call(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, B, H, N, d, dtype_enum, causal, scale,
                          hip_stream, variant));
}

int fa2_fwd_window(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                   const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2],
                   int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                   int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_fwd_window_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, B, H, N, d, dtype_enum, causal,
                                  scale, window_left, window_right, hip_stream, FA2_VARIANT_AUTO);
}

int fa2_fwd_window_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                           const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                           const int64_t l_strides[2], int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum,
                           int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                           int32_t variant) {
    FwdCall c = dense_call(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, B, H, N, d, dtype_enum, causal, scale,
                           hip_stream, variant);
    c.window_left = window_left; c.window_right = window_right;
    return fwd(c);
}

int fa2_fwd_gqa(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4], const int64_t k_strides[4],
                const int64_t v_strides[4], const int64_t o_strides[4], const int64_t l_strides[2], int32_t B, int32_t H,
                int32_t H_kv, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                int32_t window_right, void *hip_stream) {
    return fa2_fwd_gqa_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, B, H, H_kv, N, d, dtype_enum, causal,
                               scale, window_left, window_right, hip_stream, FA2_VARIANT_AUTO);
}

int fa2_fwd_gqa_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[4],
                        const int64_t k_strides[4], const int64_t v_strides[4], const int64_t o_strides[4],
                        const int64_t l_strides[2], int32_t B, int32_t H, int32_t H_kv, int32_t N, int32_t d, int32_t dtype_enum,
                        int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream,
                        int32_t variant) {
    FwdCall c = dense_call(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_strides, B, H, N, d, dtype_enum, causal, scale,
                           hip_stream, variant);
    c.window_left = window_left; c.window_right = window_right;
    c.gqa = true; c.H_kv = H_kv;
    return fwd(c);
}

int fa2_fwd_varlen(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                   const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], int64_t l_head_stride,
                   const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t d,
                   int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t dtype_enum,
                   int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_fwd_varlen_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_head_stride, cu_seqlens_q, cu_seqlens_k, B,
                                  H, d, max_seqlen_q, max_seqlen_k, total_q, total_k, dtype_enum, causal, scale, window_left,
                                  window_right, hip_stream, FA2_VARIANT_AUTO);
}

int fa2_fwd_varlen_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                           const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                           int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                           int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k,
                           int32_t dtype_enum, int32_t causal, float scale, int32_t window_left, int32_t window_right,
                           void *hip_stream, int32_t variant) {
    FwdCall c = dense_call(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, nullptr, B, H, 0, d, dtype_enum, causal, scale,
                           hip_stream, variant);
    fa2_call_packed(c, l_head_stride, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, total_q, total_k, window_left, window_right);
    return fwd(c);
}

int fa2_fwd_varlen_gqa(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                       const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], int64_t l_head_stride,
                       const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t H_kv, int32_t d,
                       int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t dtype_enum,
                       int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_fwd_varlen_gqa_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_head_stride, cu_seqlens_q,
                                      cu_seqlens_k, B, H, H_kv, d, max_seqlen_q, max_seqlen_k, total_q, total_k, dtype_enum, causal,
                                      scale, window_left, window_right, hip_stream, FA2_VARIANT_AUTO);
}

int fa2_fwd_varlen_gqa_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                               const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                               int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                               int32_t H_kv, int32_t d, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                               int32_t total_k, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                               int32_t window_right, void *hip_stream, int32_t variant) {
    FwdCall c = dense_call(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, nullptr, B, H, 0, d, dtype_enum, causal, scale,
                           hip_stream, variant);
    fa2_call_packed(c, l_head_stride, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, total_q, total_k, window_left, window_right);
    c.gqa = true; c.H_kv = H_kv;
    return fwd(c);
}

int fa2_fwd_varlen_dv(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                      const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3], int64_t l_head_stride,
                      const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H, int32_t H_kv, int32_t d,
                      int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q, int32_t total_k, int32_t dtype_enum,
                      int32_t causal, float scale, int32_t window_left, int32_t window_right, void *hip_stream) {
    return fa2_fwd_varlen_dv_variant(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, l_head_stride, cu_seqlens_q,
                                     cu_seqlens_k, B, H, H_kv, d, d_v, max_seqlen_q, max_seqlen_k, total_q, total_k, dtype_enum, causal,
                                     scale, window_left, window_right, hip_stream, FA2_VARIANT_AUTO);
}

int fa2_fwd_varlen_dv_variant(const void *Q, const void *K, const void *V, void *O, void *L, const int64_t q_strides[3],
                              const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                              int64_t l_head_stride, const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int32_t B, int32_t H,
                              int32_t H_kv, int32_t d, int32_t d_v, int32_t max_seqlen_q, int32_t max_seqlen_k, int32_t total_q,
                              int32_t total_k, int32_t dtype_enum, int32_t causal, float scale, int32_t window_left,
                              int32_t window_right, void *hip_stream, int32_t variant) {
    FwdCall c = dense_call(Q, K, V, O, L, q_strides, k_strides, v_strides, o_strides, nullptr, B, H, 0, d, dtype_enum, causal, scale,
                           hip_stream, variant);
    fa2_call_packed(c, l_head_stride, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, total_q, total_k, window_left, window_right);
    c.gqa = true; c.H_kv = H_kv;
    c.has_dv = true; c.d_v = d_v;
    return fwd(c);
}

int fa2_query_tile(int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, int32_t out4[4]) {
    return fa2_query_tile_ex(64, 8, N, d, dtype_enum, causal, out4);
}

int fa2_query_tile_ex(int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, int32_t out4[4]) {
    return fa2_query_tile_scaled(B, H, N, d, dtype_enum, causal, 1.0f, out4);
}

int fa2_query_tile_scaled(int32_t B, int32_t H, int32_t N, int32_t d, int32_t dtype_enum, int32_t causal, float scale,
                          int32_t out4[4]) {
    if (!out4) {
        fa2_set_error("out4 is null");
        return FA2_ERR_BAD_ARG;
    }
    // A contiguous (B, H, N, d) call with aligned dummy pointers: only the checks and the table are consulted.
    const int64_t st[4] = {(int64_t)H * N * d, (int64_t)N * d, d, 1}, ls[2] = {(int64_t)H * N, N};
    void *const ptr = (void *)0x1000;
    Fa2Problem p;
    Fa2Form form;
    const int rc = check_fwd(dense_call(ptr, ptr, ptr, ptr, ptr, st, st, st, st, ls, B, H, N, d, dtype_enum, causal, scale, nullptr, 0), p, form);
    if (rc != FA2_OK) return rc;
    const DenseRow &row = *dense_row(pick_variant(p));  // (every id pick_variant returns has a row)
    out4[0] = row.id; out4[1] = row.B_r; out4[2] = row.B_c; out4[3] = row.waves;
    return FA2_OK;
}

const char *fa2_version(void) { return "fa2-hip 0.2.0 gfx950"; }

const char *fa2_last_error(void) { return g_err; }

}  // extern "C"
