"""ctypes binding of libfa2_hip.so -- the only way the Python surface reaches the GPU.

Replaces the `fwd_kernel[grid](...)` Triton launch of the reference
(src/flash_attention_torch.py:59-74, src/flash_attention_wrappers.py:46-61).
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FA2_HIP_LIB points benchmarks at an alternative build (e.g. the timing-only ablation library).
LIB_PATH = os.environ.get("FA2_HIP_LIB") or os.path.join(_HERE, "libfa2_hip.so")

FA2_DTYPE_F32, FA2_DTYPE_F16, FA2_DTYPE_BF16, FA2_DTYPE_F8E5M2, FA2_DTYPE_F8E4M3, FA2_DTYPE_F64 = range(6)
VARIANT_AUTO, VARIANT_GENERIC, VARIANT_MFMA16, VARIANT_MFMA16_W8, VARIANT_MFMA32, VARIANT_MFMA16P, \
    VARIANT_MFMA16P_W8, VARIANT_MFMA16X, VARIANT_MFMA16D, VARIANT_MFMA16D_W4, VARIANT_MFMA8, \
    VARIANT_MFMA8_W4, VARIANT_MFMA16S, VARIANT_MFMA16S_W4, VARIANT_MFMA16H, VARIANT_MFMA16H_W4, \
    VARIANT_MFMA8X, VARIANT_MFMA8X_W4, VARIANT_MFMA8U, VARIANT_MFMA16K, \
    VARIANT_MFMA16K_R2K2 = range(21)
VARIANT_MFMA16K_R2K4 = 23  # 21 / 22 are the experimental MFMA16P schedules
VARIANT_A64 = 24
VARIANT_A16 = 25
VARIANT_A8 = 26
VARIANT_A64D = 27
# The variants include/fa2_fwd.h publishes -- what libfa2_hip.so runs.
VARIANTS = {"auto": VARIANT_AUTO, "generic": VARIANT_GENERIC, "mfma16": VARIANT_MFMA16, "mfma16_w8": VARIANT_MFMA16_W8,
            "mfma32": VARIANT_MFMA32, "mfma16d": VARIANT_MFMA16D, "mfma16d_w4": VARIANT_MFMA16D_W4, "mfma16h": VARIANT_MFMA16H,
            "mfma16h_w4": VARIANT_MFMA16H_W4, "mfma8x": VARIANT_MFMA8X, "mfma8x_w4": VARIANT_MFMA8X_W4, "mfma16k": VARIANT_MFMA16K,
            "mfma16k_r2k2": VARIANT_MFMA16K_R2K2, "mfma16k_r2k4": VARIANT_MFMA16K_R2K4, "a64": VARIANT_A64, "a16": VARIANT_A16, "a8": VARIANT_A8, "a64d": VARIANT_A64D}
# Experimental kernels, A/B baselines and timing-only ablations: they exist only in the experiments / ablation builds of the library
# (`make -C flash_attention_dlrs_amd/csrc experiments|abl`, csrc/fa2_experiments.h), which benchmarks/ load through FA2_HIP_LIB --
# the names are published only when such a build is the one loaded.
EXPERIMENTAL_VARIANTS = {
    "mfma16p": VARIANT_MFMA16P, "mfma16p_w8": VARIANT_MFMA16P_W8, "mfma16x": VARIANT_MFMA16X, "mfma16s": VARIANT_MFMA16S,
    "mfma16s_w4": VARIANT_MFMA16S_W4, "mfma8": VARIANT_MFMA8, "mfma8_w4": VARIANT_MFMA8_W4, "mfma8u": VARIANT_MFMA8U,
    "mfma16p_x1": VARIANT_MFMA16P + 16, "mfma16p_w8_x1": VARIANT_MFMA16P_W8 + 16,
    "abl_noexp": VARIANT_MFMA16P_W8 + 32, "abl_nosum": VARIANT_MFMA16P_W8 + 64,
    "abl_nomax": VARIANT_MFMA16P_W8 + 128, "abl_all": VARIANT_MFMA16P_W8 + 224,
    "abl_nobar": VARIANT_MFMA16P_W8 + 256, "abl_noload": VARIANT_MFMA16P_W8 + 512,
    "abl_skeleton": VARIANT_MFMA16P_W8 + 736, "abl_nobar_only": VARIANT_MFMA16P_W8 + 192 * 16,
    "mfma16p_w8_x2": VARIANT_MFMA16P_W8 + 1024, "mfma16p_x2": VARIANT_MFMA16P + 1024,
    "x_noexp": VARIANT_MFMA16X + 2048 * 1, "x_nosoftmax": VARIANT_MFMA16X + 2048 * 3,
    "x_nolds": VARIANT_MFMA16X + 2048 * 4, "x_mfma_only": VARIANT_MFMA16X + 2048 * 7,
    "x_nostage": VARIANT_MFMA16X + 2048 * 8, "x_bare": VARIANT_MFMA16X + 2048 * 15,
    "x_nobar": VARIANT_MFMA16X + 2048 * 16, "x_noload": VARIANT_MFMA16X + 2048 * 32,
    "x_nobar_noload": VARIANT_MFMA16X + 2048 * 48}
if os.path.basename(LIB_PATH) in ("libfa2_hip_exp.so", "libfa2_hip_abl.so"):
    VARIANTS.update(EXPERIMENTAL_VARIANTS)

# Every symbol include/fa2_fwd.h declares (tests/test_abi.py checks the export list against the header).
SYMBOLS = ("fa2_fwd", "fa2_fwd_variant", "fa2_query_tile", "fa2_query_tile_ex", "fa2_query_tile_scaled", "fa2_version", "fa2_last_error",
           "fa2_fwd_window", "fa2_fwd_window_variant", "fa2_fwd_varlen", "fa2_fwd_varlen_variant",
           "fa2_fwd_gqa", "fa2_fwd_gqa_variant", "fa2_fwd_varlen_gqa", "fa2_fwd_varlen_gqa_variant",
           "fa2_fwd_kvcache", "fa2_fwd_kvcache_variant", "fa2_fwd_kvcache_fp8", "fa2_fwd_kvcache_paged",
           "fa2_kvcache_workspace_bytes", "fa2_kvcache_num_splits", "fa2_kvcache_append", "fa2_fwd_kvcache_append",
           "fa2_fwd_kvcache_varlen", "fa2_kvcache_varlen_workspace_bytes", "fa2_kvcache_varlen_num_splits",
           "fa2_kvcache_append_varlen", "fa2_fwd_kvcache_varlen_append", "fa2_fwd_kvcache_mla", "fa2_kvcache_mla_num_splits",
           "fa2_fwd_kvcache_mla_fp8", "fa2_kvcache_mla_append", "fa2_kvcache_mla_append_varlen", "fa2_fwd_kvcache_mla_append",
           "fa2_fwd_kvcache_mla_varlen", "fa2_kvcache_mla_varlen_num_splits", "fa2_fwd_kvcache_mla_varlen_append",
           "fa2_fwd_kvcache_mla_sparse", "fa2_kvcache_mla_sparse_num_splits", "fa2_fwd_varlen_dv", "fa2_fwd_varlen_dv_variant",
           "fa2_mla_indexer_logits", "fa2_topk_indices", "fa2_mla_indexer_topk", "fa2_mla_indexer_workspace_bytes",
           "fa2_fwd_kvcache_mla_sparse_varlen", "fa2_kvcache_mla_sparse_varlen_num_splits", "fa2_mla_indexer_logits_varlen",
           "fa2_topk_indices_varlen", "fa2_mla_indexer_topk_varlen", "fa2_mla_indexer_varlen_workspace_bytes")
# ... and include/fa2_bwd.h
BWD_SYMBOLS = ("fa2_bwd", "fa2_bwd_variant", "fa2_bwd_window", "fa2_bwd_window_variant", "fa2_bwd_varlen", "fa2_bwd_varlen_variant",
               "fa2_bwd_gqa", "fa2_bwd_gqa_variant", "fa2_bwd_varlen_gqa", "fa2_bwd_varlen_gqa_variant",
               "fa2_bwd_varlen_dv", "fa2_bwd_varlen_dv_variant")
BWD_VARIANTS = {"auto": 0, "generic": 1, "mfma16": 2, "mfma32": 3}
# ... and the packed backward with a value head size of its own (fa2_bwd_varlen_dv): FA2_BWD_VARIANT_MFMA16DV is a variant of it alone
BWD_VARLEN_DV_VARIANTS = {"auto": 0, "generic": 1, "mfma16dv": 4}
# KV-cache decode (fa2_fwd_kvcache) has its own small variant enum, FA2_KVCACHE_VARIANT_*
KVCACHE_VARIANTS = {"auto": 0, "generic": 1, "mfma16": 2}
# ... and the latent-cache call (fa2_fwd_kvcache_mla) its own set: FA2_KVCACHE_VARIANT_MLA16 in the d 64 / 128 matrix form's place
KVCACHE_MLA_VARIANTS = {"auto": 0, "generic": 1, "mla16": 3}
# ... and the MLA indexer (fa2_mla_indexer_logits, fa2_mla_indexer_topk) its own: FA2_INDEXER_VARIANT_*
INDEXER_VARIANTS = {"auto": 0, "generic": 1, "idx16": 2}
# ... and the packed forward with a value head size of its own (fa2_fwd_varlen_dv): FA2_VARIANT_MFMA16DV is a variant of it alone
VARIANT_MFMA16DV = 28
VARLEN_DV_VARIANTS = {"auto": VARIANT_AUTO, "generic": VARIANT_GENERIC, "mfma16dv": VARIANT_MFMA16DV}
KVCACHE_MAX_SPLITS = 128

_lib = None


class Fa2LibraryMissing(ImportError):
    pass


def lib():
    """Load the C-ABI library.  No fallback: a missing build is an error."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Fa2LibraryMissing(
                f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C flash_attention_dlrs_amd/csrc`. There is no CPU fallback.")
        l = ctypes.CDLL(LIB_PATH)
        i64p = ctypes.POINTER(ctypes.c_int64)
        vp = ctypes.c_void_p
        common = [vp, vp, vp, vp, vp, i64p, i64p, i64p, i64p, i64p] + [ctypes.c_int32] * 6 + [ctypes.c_float, vp]
        l.fa2_fwd.restype = ctypes.c_int
        l.fa2_fwd.argtypes = common
        l.fa2_fwd_variant.restype = ctypes.c_int
        l.fa2_fwd_variant.argtypes = common + [ctypes.c_int32]
        # second prototype of the same entry for the hot path: the five stride pointers as plain addresses into ONE
        # int64 array (fa2_fwd below), which saves building five ctypes arrays per launch
        l.fwd_variant_addr = ctypes.CFUNCTYPE(ctypes.c_int, *([vp] * 10 + [ctypes.c_int32] * 6 + [ctypes.c_float, vp, ctypes.c_int32]))(
            ("fa2_fwd_variant", l))
        # local attention: window_left, window_right after scale
        win = common[:-1] + [ctypes.c_int32, ctypes.c_int32, vp]
        l.fa2_fwd_window.restype = ctypes.c_int
        l.fa2_fwd_window.argtypes = win
        l.fa2_fwd_window_variant.restype = ctypes.c_int
        l.fa2_fwd_window_variant.argtypes = win + [ctypes.c_int32]
        # variable-length (packed): 3-element strides, L head stride, cu_seqlens, B H d, max_seqlen, total, dtype causal, scale, window
        vl = [vp] * 5 + [i64p] * 4 + [ctypes.c_int64, vp, vp] + [ctypes.c_int32] * 9 + [ctypes.c_float] + [ctypes.c_int32] * 2 + [vp]
        l.fa2_fwd_varlen.restype = ctypes.c_int
        l.fa2_fwd_varlen.argtypes = vl
        l.fa2_fwd_varlen_variant.restype = ctypes.c_int
        l.fa2_fwd_varlen_variant.argtypes = vl + [ctypes.c_int32]
        bvl = [vp] * 10 + [i64p] * 8 + [ctypes.c_int64, vp, vp] + [ctypes.c_int32] * 9 + [ctypes.c_float] + [ctypes.c_int32] * 2 + [vp]
        l.fa2_bwd_varlen.restype = ctypes.c_int
        l.fa2_bwd_varlen.argtypes = bvl
        l.fa2_bwd_varlen_variant.restype = ctypes.c_int
        l.fa2_bwd_varlen_variant.argtypes = bvl + [ctypes.c_int32]
        l.fa2_query_tile.restype = ctypes.c_int
        l.fa2_query_tile.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]
        l.fa2_query_tile_ex.restype = ctypes.c_int
        l.fa2_query_tile_ex.argtypes = [ctypes.c_int32] * 6 + [ctypes.POINTER(ctypes.c_int32)]
        l.fa2_query_tile_scaled.restype = ctypes.c_int
        l.fa2_query_tile_scaled.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_float, ctypes.POINTER(ctypes.c_int32)]
        bwd = [vp] * 10 + [i64p] * 9 + [ctypes.c_int32] * 6 + [ctypes.c_float, vp]
        l.fa2_bwd.restype = ctypes.c_int
        l.fa2_bwd.argtypes = bwd
        l.fa2_bwd_variant.restype = ctypes.c_int
        l.fa2_bwd_variant.argtypes = bwd + [ctypes.c_int32]
        bwd_win = bwd[:-1] + [ctypes.c_int32, ctypes.c_int32, vp]
        l.fa2_bwd_window.restype = ctypes.c_int
        l.fa2_bwd_window.argtypes = bwd_win
        l.fa2_bwd_window_variant.restype = ctypes.c_int
        l.fa2_bwd_window_variant.argtypes = bwd_win + [ctypes.c_int32]
        # grouped-query attention: H_kv after H (dense: the window sides after scale as well)
        gqa = common[:10] + [ctypes.c_int32] * 7 + [ctypes.c_float, ctypes.c_int32, ctypes.c_int32, vp]
        l.fa2_fwd_gqa.restype = ctypes.c_int
        l.fa2_fwd_gqa.argtypes = gqa
        l.fa2_fwd_gqa_variant.restype = ctypes.c_int
        l.fa2_fwd_gqa_variant.argtypes = gqa + [ctypes.c_int32]
        bgqa = bwd[:19] + [ctypes.c_int32] * 7 + [ctypes.c_float, ctypes.c_int32, ctypes.c_int32, vp]
        l.fa2_bwd_gqa.restype = ctypes.c_int
        l.fa2_bwd_gqa.argtypes = bgqa
        l.fa2_bwd_gqa_variant.restype = ctypes.c_int
        l.fa2_bwd_gqa_variant.argtypes = bgqa + [ctypes.c_int32]
        vlg = vl[:12] + [ctypes.c_int32] * 10 + vl[21:]
        l.fa2_fwd_varlen_gqa.restype = ctypes.c_int
        l.fa2_fwd_varlen_gqa.argtypes = vlg
        l.fa2_fwd_varlen_gqa_variant.restype = ctypes.c_int
        l.fa2_fwd_varlen_gqa_variant.argtypes = vlg + [ctypes.c_int32]
        # a value head size of its own: d_v after d
        vld = vl[:12] + [ctypes.c_int32] * 11 + vl[21:]
        l.fa2_fwd_varlen_dv.restype = ctypes.c_int
        l.fa2_fwd_varlen_dv.argtypes = vld
        l.fa2_fwd_varlen_dv_variant.restype = ctypes.c_int
        l.fa2_fwd_varlen_dv_variant.argtypes = vld + [ctypes.c_int32]
        bvlg = bvl[:21] + [ctypes.c_int32] * 10 + bvl[30:]
        l.fa2_bwd_varlen_gqa.restype = ctypes.c_int
        l.fa2_bwd_varlen_gqa.argtypes = bvlg
        l.fa2_bwd_varlen_gqa_variant.restype = ctypes.c_int
        l.fa2_bwd_varlen_gqa_variant.argtypes = bvlg + [ctypes.c_int32]
        bvld = bvl[:21] + [ctypes.c_int32] * 11 + bvl[30:]  # d_v after d
        l.fa2_bwd_varlen_dv.restype = ctypes.c_int
        l.fa2_bwd_varlen_dv.argtypes = bvld
        l.fa2_bwd_varlen_dv_variant.restype = ctypes.c_int
        l.fa2_bwd_varlen_dv_variant.argtypes = bvld + [ctypes.c_int32]
        # KV-cache decode: 4-element strides, L strides, cache_seqlens, B H H_kv N_q S_k d dtype causal, scale, window, num_splits,
        # workspace + its size, stream
        kvc = [vp] * 5 + [i64p] * 5 + [vp] + [ctypes.c_int32] * 8 + [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, vp]
        l.fa2_fwd_kvcache.restype = ctypes.c_int
        l.fa2_fwd_kvcache.argtypes = kvc
        l.fa2_fwd_kvcache_variant.restype = ctypes.c_int
        l.fa2_fwd_kvcache_variant.argtypes = kvc + [ctypes.c_int32]
        # ... over an fp8 cache: the two descales and their (B, H_kv) strides after cache_seqlens, kv_dtype after dtype, variant
        # before the stream
        l.fa2_fwd_kvcache_fp8.restype = ctypes.c_int
        l.fa2_fwd_kvcache_fp8.argtypes = [vp] * 5 + [i64p] * 5 + [vp, vp, vp, i64p, i64p] + [ctypes.c_int32] * 9 + [ctypes.c_float] + \
            [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # ... over a paged cache: block_table and its row stride after cache_seqlens; num_blocks, page_size, max_blocks in S_k's place
        l.fa2_fwd_kvcache_paged.restype = ctypes.c_int
        l.fa2_fwd_kvcache_paged.argtypes = [vp] * 5 + [i64p] * 5 + [vp, vp, ctypes.c_int64, vp, vp, i64p, i64p] + [ctypes.c_int32] * 11 + \
            [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # the cache append: cache + strides, table + stride, new tokens + strides, lengths in / out, descales + strides, rotary tables +
        # row strides, S_rot rotary_dim interleaved, Q q_rot q_strides, H N_q q_pos_per_row, B H_kv N_new S_k num_blocks page_size
        # max_blocks d dtype kv_dtype, stream
        l.fa2_kvcache_append.restype = ctypes.c_int
        l.fa2_kvcache_append.argtypes = [vp, vp, i64p, i64p, vp, ctypes.c_int64, vp, vp, i64p, i64p, vp, vp, vp, vp, i64p, i64p, vp, vp,
                                         ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [vp, vp, i64p] + [ctypes.c_int32] * 13 + [vp]
        # ... fused with the decode attention that follows
        l.fa2_fwd_kvcache_append.restype = ctypes.c_int
        l.fa2_fwd_kvcache_append.argtypes = [vp] * 5 + [i64p] * 5 + [vp, vp, vp, ctypes.c_int64, vp, vp, i64p, i64p, vp, vp, i64p, i64p, vp, vp,
                                             ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [vp] + [ctypes.c_int32] * 13 + \
            [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # packed queries over the cache: 3-element Q / O strides, L head stride, cu_seqlens_q, cache_seqlens, table + stride, descales
        # + strides, B H H_kv total_q max_seqlen_q S_k num_blocks page_size max_blocks d dtype kv_dtype causal, scale, window,
        # num_splits, workspace + its size, variant, stream
        l.fa2_fwd_kvcache_varlen.restype = ctypes.c_int
        l.fa2_fwd_kvcache_varlen.argtypes = [vp] * 5 + [i64p] * 4 + [ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp, vp, i64p, i64p] + \
            [ctypes.c_int32] * 13 + [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # the packed append: fa2_kvcache_append's order with 3-element k_new / v_new / Q strides, cu_seqlens_new before cache_seqlens,
        # no N_q, and total_new max_seqlen_new in N_new's place
        l.fa2_kvcache_append_varlen.restype = ctypes.c_int
        l.fa2_kvcache_append_varlen.argtypes = [vp, vp, i64p, i64p, vp, ctypes.c_int64, vp, vp, i64p, i64p, vp, vp, vp, vp, vp, i64p, i64p, vp,
                                                vp, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [vp, vp, i64p] + \
            [ctypes.c_int32] * 13 + [vp]
        # ... fused with the packed-query attention: fa2_fwd_kvcache_varlen's order with seqlens_out after cache_seqlens and, after the
        # descales, k_new v_new + strides, rotary tables + row strides, S_rot rotary_dim interleaved, q_rot
        l.fa2_fwd_kvcache_varlen_append.restype = ctypes.c_int
        l.fa2_fwd_kvcache_varlen_append.argtypes = [vp] * 5 + [i64p] * 4 + [ctypes.c_int64, vp, vp, vp, vp, ctypes.c_int64, vp, vp, i64p, i64p,
                                                    vp, vp, i64p, i64p, vp, vp, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + \
            [vp] + [ctypes.c_int32] * 13 + [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        l.fa2_kvcache_varlen_workspace_bytes.restype = ctypes.c_int64
        l.fa2_kvcache_varlen_workspace_bytes.argtypes = [ctypes.c_int32] * 4
        l.fa2_kvcache_varlen_num_splits.restype = ctypes.c_int32
        l.fa2_kvcache_varlen_num_splits.argtypes = [ctypes.c_int32] * 8
        # fa2_fwd_kvcache_paged's order without the descales, d_v after d, no kv_dtype_enum
        l.fa2_fwd_kvcache_mla.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla.argtypes = [vp] * 5 + [i64p] * 5 + [vp, vp, ctypes.c_int64] + [ctypes.c_int32] * 11 + \
            [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # ... over an fp8 latent cache: fa2_fwd_kvcache_paged's order with d_v after d
        l.fa2_fwd_kvcache_mla_fp8.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla_fp8.argtypes = [vp] * 5 + [i64p] * 5 + [vp, vp, ctypes.c_int64, vp, vp, i64p, i64p] + [ctypes.c_int32] * 12 + \
            [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        l.fa2_kvcache_mla_num_splits.restype = ctypes.c_int32
        l.fa2_kvcache_mla_num_splits.argtypes = [ctypes.c_int32] * 8
        # the latent-cache append: fa2_kvcache_append's order with one cache tensor and one descale, c_new / pe_new in k_new / v_new's
        # place, d_v after d
        l.fa2_kvcache_mla_append.restype = ctypes.c_int
        l.fa2_kvcache_mla_append.argtypes = [vp, i64p, vp, ctypes.c_int64, vp, vp, i64p, i64p, vp, vp, vp, i64p, vp, vp, ctypes.c_int64,
                                             ctypes.c_int64] + [ctypes.c_int32] * 3 + [vp, vp, i64p] + [ctypes.c_int32] * 14 + [vp]
        # ... packed: cu_seqlens_new before cache_seqlens, no N_q, total_new max_seqlen_new in N_new's place
        l.fa2_kvcache_mla_append_varlen.restype = ctypes.c_int
        l.fa2_kvcache_mla_append_varlen.argtypes = [vp, i64p, vp, ctypes.c_int64, vp, vp, i64p, i64p, vp, vp, vp, vp, i64p, vp, vp,
                                                    ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [vp, vp, i64p] + \
            [ctypes.c_int32] * 14 + [vp]
        # ... fused with the latent-cache decode: Q KV O L + their strides, lengths in / out, table + stride, descale + strides,
        # c_new pe_new + strides, rotary tables + row strides, S_rot rotary_dim interleaved, q_rot, B H H_kv N_q N_new S_k num_blocks
        # page_size max_blocks d d_v dtype kv_dtype causal, scale, window, num_splits, workspace + its size, variant, stream
        l.fa2_fwd_kvcache_mla_append.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla_append.argtypes = [vp] * 4 + [i64p] * 4 + [vp, vp, vp, ctypes.c_int64, vp, i64p, vp, vp, i64p, i64p, vp, vp,
                                                 ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + [vp] + [ctypes.c_int32] * 14 + \
            [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # packed queries over the latent cache: fa2_fwd_kvcache_varlen's order with one cache tensor and one descale, d_v after d
        l.fa2_fwd_kvcache_mla_varlen.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla_varlen.argtypes = [vp] * 4 + [i64p] * 3 + [ctypes.c_int64, vp, vp, vp, ctypes.c_int64, vp, i64p] + \
            [ctypes.c_int32] * 14 + [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        l.fa2_kvcache_mla_varlen_num_splits.restype = ctypes.c_int32
        l.fa2_kvcache_mla_varlen_num_splits.argtypes = [ctypes.c_int32] * 9
        # ... fused with the packed latent-cache append: seqlens_out after cache_seqlens and, after the descale, c_new pe_new + strides,
        # rotary tables + row strides, S_rot rotary_dim interleaved, q_rot
        l.fa2_fwd_kvcache_mla_varlen_append.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla_varlen_append.argtypes = [vp] * 4 + [i64p] * 3 + [ctypes.c_int64, vp, vp, vp, vp, ctypes.c_int64, vp, i64p, vp,
                                                        vp, i64p, i64p, vp, vp, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int32] * 3 + \
            [vp] + [ctypes.c_int32] * 14 + [ctypes.c_float] + [ctypes.c_int32] * 3 + [vp, ctypes.c_int64, ctypes.c_int32, vp]
        # key lists over the latent cache: fa2_fwd_kvcache_mla_fp8's order with indices, their strides and topk after cache_seqlens, no
        # causal and no window sides
        l.fa2_fwd_kvcache_mla_sparse.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla_sparse.argtypes = [vp] * 5 + [i64p] * 5 + [vp, vp, i64p, ctypes.c_int32, vp, ctypes.c_int64, vp, vp, i64p,
                                                                         i64p] + [ctypes.c_int32] * 11 + \
            [ctypes.c_float, ctypes.c_int32, vp, ctypes.c_int64, ctypes.c_int32, vp]
        l.fa2_kvcache_mla_sparse_num_splits.restype = ctypes.c_int32
        l.fa2_kvcache_mla_sparse_num_splits.argtypes = [ctypes.c_int32] * 8
        # the MLA indexer: five tensors, their five stride arrays, cache_seqlens, the table and its stride, eight sizes, the two dtypes,
        # causal; then variant (scores alone) or topk, indices, their strides, variant (both); the selection alone has a list of its own
        idx = [vp] * 5 + [i64p] * 5 + [vp, vp, ctypes.c_int64] + [ctypes.c_int32] * 11
        l.fa2_mla_indexer_logits.restype = ctypes.c_int
        l.fa2_mla_indexer_logits.argtypes = idx + [ctypes.c_int32, vp]
        l.fa2_mla_indexer_topk.restype = ctypes.c_int
        l.fa2_mla_indexer_topk.argtypes = idx + [ctypes.c_int32, vp, i64p, ctypes.c_int32, vp]
        l.fa2_topk_indices.restype = ctypes.c_int
        l.fa2_topk_indices.argtypes = [vp, i64p, vp] + [ctypes.c_int32] * 5 + [vp, i64p, vp]
        l.fa2_mla_indexer_workspace_bytes.restype = ctypes.c_int64
        l.fa2_mla_indexer_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        # key lists of packed queries: fa2_fwd_kvcache_mla_sparse's order with 3-element Q / O / index strides, the L head stride,
        # cu_seqlens_q before cache_seqlens, and total_q max_seqlen_q in N_q's place
        l.fa2_fwd_kvcache_mla_sparse_varlen.restype = ctypes.c_int
        l.fa2_fwd_kvcache_mla_sparse_varlen.argtypes = [vp] * 5 + [i64p] * 4 + [ctypes.c_int64, vp, vp, vp, i64p, ctypes.c_int32, vp,
                                                                                ctypes.c_int64, vp, vp, i64p, i64p] + \
            [ctypes.c_int32] * 12 + [ctypes.c_float, ctypes.c_int32, vp, ctypes.c_int64, ctypes.c_int32, vp]
        l.fa2_kvcache_mla_sparse_varlen_num_splits.restype = ctypes.c_int32
        l.fa2_kvcache_mla_sparse_varlen_num_splits.argtypes = [ctypes.c_int32] * 7
        # the packed indexer: the fixed calls' order with cu_seqlens_q before cache_seqlens and total_q max_seqlen_q in N_q's place
        idxv = [vp] * 5 + [i64p] * 5 + [vp, vp, vp, ctypes.c_int64] + [ctypes.c_int32] * 12
        l.fa2_mla_indexer_logits_varlen.restype = ctypes.c_int
        l.fa2_mla_indexer_logits_varlen.argtypes = idxv + [ctypes.c_int32, vp]
        l.fa2_mla_indexer_topk_varlen.restype = ctypes.c_int
        l.fa2_mla_indexer_topk_varlen.argtypes = idxv + [ctypes.c_int32, vp, i64p, ctypes.c_int32, vp]
        l.fa2_topk_indices_varlen.restype = ctypes.c_int
        l.fa2_topk_indices_varlen.argtypes = [vp, i64p, vp, vp] + [ctypes.c_int32] * 6 + [vp, i64p, vp]
        l.fa2_mla_indexer_varlen_workspace_bytes.restype = ctypes.c_int64
        l.fa2_mla_indexer_varlen_workspace_bytes.argtypes = [ctypes.c_int32] * 2
        l.fa2_kvcache_workspace_bytes.restype = ctypes.c_int64
        l.fa2_kvcache_workspace_bytes.argtypes = [ctypes.c_int32] * 5
        l.fa2_kvcache_num_splits.restype = ctypes.c_int32
        l.fa2_kvcache_num_splits.argtypes = [ctypes.c_int32] * 7
        l.bwd_variant_addr = ctypes.CFUNCTYPE(ctypes.c_int, *([vp] * 19 + [ctypes.c_int32] * 6 + [ctypes.c_float, vp, ctypes.c_int32]))(
            ("fa2_bwd_variant", l))
        l.fa2_version.restype = ctypes.c_char_p
        l.fa2_last_error.restype = ctypes.c_char_p
        _lib = l
    return _lib


def version():
    return lib().fa2_version().decode()


def query_tile(N, d, dtype_enum, causal=False, B=None, H=None, scale=None):
    """(variant, B_r, B_c, waves) the static table picks; the choice depends on the grid size, so pass B and H for the
    variant an actual (B, H, N, d) launch takes (default: a large grid, B = 64, H = 8) -- and, for f16, on the softmax scale
    (default 1, the reference's)"""
    out = (ctypes.c_int32 * 4)()
    if scale is not None:
        rc = lib().fa2_query_tile_scaled(64 if B is None else B, 8 if H is None else H, N, d, dtype_enum, int(bool(causal)), float(scale), out)
    elif B is None or H is None:
        rc = lib().fa2_query_tile(N, d, dtype_enum, int(bool(causal)), out)
    else:
        rc = lib().fa2_query_tile_ex(B, H, N, d, dtype_enum, int(bool(causal)), out)
    if rc != 0:
        _raise(rc)
    return tuple(out)


def _raise(rc):
    msg = lib().fa2_last_error().decode()
    if rc == -2:
        raise TypeError(f"fa2_fwd: {msg}")           # reference: TypeError for unsupported dtype (torch.py:18)
    if rc in (-1, -3):
        raise ValueError(f"fa2_fwd: {msg}")          # reference: ValueError for bad shapes (torch.py:28-32)
    raise RuntimeError(f"fa2_fwd rc={rc}: {msg}")


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _raw_stream(index):
    """Handle of torch's current stream on device `index`."""
    try:
        return torch._C._cuda_getCurrentRawStream(index)
    except AttributeError:  # older / newer torch without the private accessor
        return torch.cuda.current_stream(index).cuda_stream


def fa2_fwd(Q, K, V, O, L, dtype_enum, causal=False, scale=1.0, variant=VARIANT_AUTO, window=None):
    """Launch the forward on the current stream of Q's device.  Tensors are (B, H, N, d) with
    arbitrary strides; O (B, H, N, d) and L (B, H, N, 1) are pre-allocated by the caller exactly as
    the reference's host glue does (torch.py:50-51).  window = (left, right): local attention through
    fa2_fwd_window_variant (include/fa2_fwd.h); None is the plain call."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N, d = Q.shape
    LB, LH = L.stride(0), L.stride(1)
    if K.shape[1] != H:  # grouped-query: K and V with H_kv heads (fa2_fwd_gqa_variant)
        wl, wr = (-1, -1) if window is None else (int(w) for w in window)
        with torch.cuda.device(Q.device):
            rc = lib().fa2_fwd_gqa_variant(
                Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
                _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((LB, LH)),
                B, H, K.shape[1], N, d, int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index),
                int(variant))
        if rc != 0:
            _raise(rc)
        return
    if window is not None:
        wl, wr = (int(w) for w in window)
        with torch.cuda.device(Q.device):
            rc = lib().fa2_fwd_window_variant(
                Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
                _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((LB, LH)),
                B, H, N, d, int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
        if rc != 0:
            _raise(rc)
        return

    def launch():
        # one int64 array for the 18 strides (five ctypes arrays cost ~2 us), raw stream handle without the Stream object
        st = (ctypes.c_int64 * 18)(*Q.stride(), *K.stride(), *V.stride(), *O.stride(), LB, LH)
        base = ctypes.addressof(st)
        return lib().fwd_variant_addr(
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            base, base + 32, base + 64, base + 96, base + 128,
            B, H, N, d, int(dtype_enum), int(bool(causal)), float(scale), _raw_stream(Q.device.index), int(variant))
    # the library launches on the CURRENT HIP device: switch only if it is not the tensors' one (the device guard
    # costs several microseconds of the ~15 a small launch takes on the host)
    if torch.cuda.current_device() == Q.device.index:
        rc = launch()
    else:
        with torch.cuda.device(Q.device):
            rc = launch()
    if rc != 0:
        _raise(rc)


def fa2_bwd(Q, K, V, O, dO, L, dQ, dK, dV, D, dtype_enum, causal=False, scale=1.0, variant=0, window=None):
    """Launch the backward (include/fa2_bwd.h) on the current stream of Q's device: the counterpart of the
    reference's bwd_D_kernel + bwd_kernel launches (torch.py:124-155).  All buffers, the float32 scratch D
    (2, B, H, N, 1) included, are allocated by the caller as the reference's glue does (torch.py:101-105).
    window = (left, right): local attention through fa2_bwd_window_variant; None is the plain call."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N, d = Q.shape
    assert D.is_contiguous() and D.numel() == 2 * B * H * N
    if K.shape[1] != H:  # grouped-query: K, V, dK, dV with H_kv heads (fa2_bwd_gqa_variant)
        wl, wr = (-1, -1) if window is None else (int(w) for w in window)
        with torch.cuda.device(Q.device):
            rc = lib().fa2_bwd_gqa_variant(
                Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
                dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D.data_ptr(),
                *(_i64(t.stride()) for t in (Q, K, V, O, dO, dQ, dK, dV)), _i64((L.stride(0), L.stride(1))),
                B, H, K.shape[1], N, d, int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index),
                int(variant))
        if rc != 0:
            _raise(rc)
        return
    if window is not None:
        wl, wr = (int(w) for w in window)
        with torch.cuda.device(Q.device):
            rc = lib().fa2_bwd_window_variant(
                Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
                dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D.data_ptr(),
                *(_i64(t.stride()) for t in (Q, K, V, O, dO, dQ, dK, dV)), _i64((L.stride(0), L.stride(1))),
                B, H, N, d, int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
        if rc != 0:
            _raise(rc)
        return

    def launch():
        st = (ctypes.c_int64 * 34)(*Q.stride(), *K.stride(), *V.stride(), *O.stride(), *dO.stride(), *dQ.stride(),
                                    *dK.stride(), *dV.stride(), L.stride(0), L.stride(1))
        base = ctypes.addressof(st)
        return lib().bwd_variant_addr(
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
            dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D.data_ptr(),
            *(base + 32 * k for k in range(9)),
            B, H, N, d, int(dtype_enum), int(bool(causal)), float(scale), _raw_stream(Q.device.index), int(variant))
    if torch.cuda.current_device() == Q.device.index:
        rc = launch()
    else:
        with torch.cuda.device(Q.device):
            rc = launch()
    if rc != 0:
        _raise(rc)


def fa2_fwd_varlen(Q, K, V, O, L, cu_q, cu_k, max_q, max_k, dtype_enum, causal=False, scale=1.0, window=None,
                   variant=VARIANT_AUTO):
    """Launch the variable-length forward (include/fa2_fwd.h fa2_fwd_varlen_variant) on the current stream of Q's device.
    Q (total_q, H, d), K / V (total_k, H, d), O like Q, L (H, total_q) with unit token stride; cu_q / cu_k int32 on the
    device.  window = (left, right) raw sides (-1 unbounded) or None."""
    total_q, H, d = Q.shape
    wl, wr = (-1, -1) if window is None else (int(w) for w in window)
    if K.shape[1] != H:  # grouped-query: K and V (total_k, H_kv, d)
        with torch.cuda.device(Q.device):
            rc = lib().fa2_fwd_varlen_gqa_variant(
                Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
                _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), L.stride(0),
                cu_q.data_ptr(), cu_k.data_ptr(), cu_q.numel() - 1, H, K.shape[1], d, int(max_q), int(max_k), total_q,
                K.shape[0], int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
        if rc != 0:
            _raise(rc)
        return
    with torch.cuda.device(Q.device):
        rc = lib().fa2_fwd_varlen_variant(
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), L.stride(0),
            cu_q.data_ptr(), cu_k.data_ptr(), cu_q.numel() - 1, H, d, int(max_q), int(max_k), total_q, K.shape[0],
            int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
    if rc != 0:
        _raise(rc)


def fa2_fwd_varlen_dv(Q, K, V, O, L, cu_q, cu_k, max_q, max_k, dtype_enum, causal=False, scale=1.0, window=None,
                      variant=VARIANT_AUTO):
    """Launch the variable-length forward with a value head size of its own (include/fa2_fwd.h fa2_fwd_varlen_dv_variant) on the
    current stream of Q's device.  Q (total_q, H, d), K (total_k, H_kv, d), V (total_k, H_kv, d_v), O (total_q, H, d_v), any
    strides; L (H, total_q) with unit token stride; cu_q / cu_k int32 on the device.  window = (left, right) raw sides or None."""
    total_q, H, d = Q.shape
    wl, wr = (-1, -1) if window is None else (int(w) for w in window)
    with torch.cuda.device(Q.device):
        rc = lib().fa2_fwd_varlen_dv_variant(
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), L.stride(0),
            cu_q.data_ptr(), cu_k.data_ptr(), cu_q.numel() - 1, H, K.shape[1], d, V.shape[2], int(max_q), int(max_k), total_q,
            K.shape[0], int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
    if rc != 0:
        _raise(rc)


def fa2_bwd_varlen(Q, K, V, O, dO, L, dQ, dK, dV, D, cu_q, cu_k, max_q, max_k, dtype_enum, causal=False, scale=1.0,
                   window=None, variant=0):
    """Launch the variable-length backward (include/fa2_bwd.h fa2_bwd_varlen_variant).  D: contiguous scratch of
    2 * H * total_q float32 (float64 for fp64)."""
    total_q, H, d = Q.shape
    assert D.is_contiguous() and D.numel() == 2 * H * total_q
    wl, wr = (-1, -1) if window is None else (int(w) for w in window)
    if K.shape[1] != H:  # grouped-query: K, V, dK, dV (total_k, H_kv, d)
        with torch.cuda.device(Q.device):
            rc = lib().fa2_bwd_varlen_gqa_variant(
                Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
                dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D.data_ptr(),
                *(_i64(t.stride()) for t in (Q, K, V, O, dO, dQ, dK, dV)), L.stride(0),
                cu_q.data_ptr(), cu_k.data_ptr(), cu_q.numel() - 1, H, K.shape[1], d, int(max_q), int(max_k), total_q,
                K.shape[0], int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
        if rc != 0:
            _raise(rc)
        return
    with torch.cuda.device(Q.device):
        rc = lib().fa2_bwd_varlen_variant(
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
            dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D.data_ptr(),
            *(_i64(t.stride()) for t in (Q, K, V, O, dO, dQ, dK, dV)), L.stride(0),
            cu_q.data_ptr(), cu_k.data_ptr(), cu_q.numel() - 1, H, d, int(max_q), int(max_k), total_q, K.shape[0],
            int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
    if rc != 0:
        _raise(rc)


def fa2_bwd_varlen_dv(Q, K, V, O, dO, L, dQ, dK, dV, D, cu_q, cu_k, max_q, max_k, dtype_enum, causal=False, scale=1.0,
                      window=None, variant=0):
    """Launch the variable-length backward with a value head size of its own (include/fa2_bwd.h fa2_bwd_varlen_dv_variant).
    Q, dQ (total_q, H, d), K, dK (total_k, H_kv, d), V, dV (total_k, H_kv, d_v), O, dO (total_q, H, d_v), any strides; L (H, total_q)
    with unit token stride; D: contiguous scratch of 2 * H * total_q float32 (float64 for fp64)."""
    total_q, H, d = Q.shape
    assert D.is_contiguous() and D.numel() == 2 * H * total_q
    wl, wr = (-1, -1) if window is None else (int(w) for w in window)
    with torch.cuda.device(Q.device):
        rc = lib().fa2_bwd_varlen_dv_variant(
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), L.data_ptr(),
            dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), D.data_ptr(),
            *(_i64(t.stride()) for t in (Q, K, V, O, dO, dQ, dK, dV)), L.stride(0),
            cu_q.data_ptr(), cu_k.data_ptr(), cu_q.numel() - 1, H, K.shape[1], d, V.shape[2], int(max_q), int(max_k), total_q,
            K.shape[0], int(dtype_enum), int(bool(causal)), float(scale), wl, wr, _raw_stream(Q.device.index), int(variant))
    if rc != 0:
        _raise(rc)


def _window_sides(window):
    if window is None:
        return -1, -1
    wl, wr = window
    return int(wl), int(wr)


def _workspace_args(workspace):
    """(pointer, size in bytes) of the split workspace, (None, 0) without one."""
    return (None, 0) if workspace is None else (workspace.data_ptr(), workspace.numel() * workspace.element_size())


def _descale_args(k_descale, v_descale):
    """(k pointer, v pointer, k strides, v strides) of the fp8 descales, None where one is not given."""
    kd_ptr, kd_st = (None, None) if k_descale is None else (k_descale.data_ptr(), _i64(k_descale.stride()))
    vd_ptr, vd_st = (None, None) if v_descale is None else (v_descale.data_ptr(), _i64(v_descale.stride()))
    return kd_ptr, vd_ptr, kd_st, vd_st


def _table_args(K, block_table):
    """(table pointer, row stride, S_k, num_blocks, page_size, max_blocks): S_k of the contiguous cache K, or the pool K's sizes."""
    if block_table is None:
        return None, 0, K.shape[2], 0, 0, 0
    return block_table.data_ptr(), block_table.stride(0), 0, K.shape[0], K.shape[2], block_table.shape[1]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(fn, anchor, *args):
    """Call the entry point fn, args in the header's order, with anchor's device current; raise what it refuses."""
    with torch.cuda.device(anchor.device.index):  # (the index: the context is built from it faster than from the torch.device)
        rc = fn(*args)
    if rc != 0:
        _raise(rc)


def kvcache_num_splits(B, H, H_kv, N_q, S_k, d, dtype_enum):
    """What num_splits = 0 resolves to for a decode call of this shape (fa2_kvcache_num_splits): a host heuristic on the capacity."""
    return int(lib().fa2_kvcache_num_splits(B, H, H_kv, N_q, S_k, d, int(dtype_enum)))


def kvcache_workspace_bytes(B, H, N_q, d, num_splits):
    """Bytes of fp32 workspace a decode call with this num_splits needs (fa2_kvcache_workspace_bytes); 0 for num_splits <= 1."""
    return int(lib().fa2_kvcache_workspace_bytes(B, H, N_q, d, num_splits))


def fa2_fwd_kvcache(Q, K, V, O, L, cache_seqlens, dtype_enum, causal=False, scale=1.0, window=None, num_splits=0, workspace=None,
                    variant=0):
    """Launch decode attention over a padded KV cache (include/fa2_fwd.h fa2_fwd_kvcache_variant) on the current stream of Q's
    device.  Q, O (B, H, N_q, d), K / V (B, H_kv, S_k, d) with any strides, L (B, H, N_q) with unit last stride; cache_seqlens int32
    (B,) on the device or None; workspace: a tensor of at least kvcache_workspace_bytes(...) bytes when num_splits resolves to more
    than 1, else None."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    _launch(lib().fa2_fwd_kvcache_variant, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            None if cache_seqlens is None else cache_seqlens.data_ptr(), B, H, K.shape[1], N_q, K.shape[2], d, int(dtype_enum),
            int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            _raw_stream(Q.device.index), int(variant))


def fa2_fwd_kvcache_fp8(Q, K, V, O, L, cache_seqlens, dtype_enum, kv_dtype_enum, k_descale=None, v_descale=None, causal=False, scale=1.0,
                        window=None, num_splits=0, workspace=None, variant=0):
    """Launch decode attention over an fp8 KV cache (include/fa2_fwd.h fa2_fwd_kvcache_fp8) on the current stream of Q's device.
    As fa2_fwd_kvcache, with K / V in kv_dtype_enum (an fp8 format) and k_descale / v_descale: float32 tensors on the device viewed
    as (B, H_kv) (expanded views are fine: their strides are passed on), or None for 1."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    _launch(lib().fa2_fwd_kvcache_fp8, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            None if cache_seqlens is None else cache_seqlens.data_ptr(), *_descale_args(k_descale, v_descale), B, H, K.shape[1], N_q, K.shape[2], d, int(dtype_enum),
            int(kv_dtype_enum), int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            int(variant), _raw_stream(Q.device.index))


def fa2_fwd_kvcache_paged(Q, K, V, O, L, block_table, cache_seqlens, dtype_enum, kv_dtype_enum, k_descale=None, v_descale=None,
                          causal=False, scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch decode attention over a paged KV cache (include/fa2_fwd.h fa2_fwd_kvcache_paged) on the current stream of Q's device.
    As fa2_fwd_kvcache_fp8, with K / V the page pool (num_blocks, H_kv, page_size, d), any strides, and block_table int32
    (B, max_blocks) on the device with unit stride in its last axis; kv_dtype_enum == dtype_enum (and no descales) for a pool in
    Q's dtype.  The kernels clamp table entries into the pool; nothing is validated here."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    _launch(lib().fa2_fwd_kvcache_paged, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            None if cache_seqlens is None else cache_seqlens.data_ptr(), block_table.data_ptr(), block_table.stride(0), *_descale_args(k_descale, v_descale),
            B, H, K.shape[1], N_q, K.shape[0], K.shape[2], block_table.shape[1], d, int(dtype_enum), int(kv_dtype_enum),
            int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            int(variant), _raw_stream(Q.device.index))


def kvcache_mla_num_splits(B, H, H_kv, N_q, S_k, d, d_v, dtype_enum):
    """What num_splits = 0 resolves to for a latent-cache decode call of this shape (fa2_kvcache_mla_num_splits)."""
    return int(lib().fa2_kvcache_mla_num_splits(B, H, H_kv, N_q, S_k, d, d_v, int(dtype_enum)))


def fa2_fwd_kvcache_mla(Q, K, V, O, L, cache_seqlens, dtype_enum, block_table=None, causal=False, scale=1.0, window=None, num_splits=0,
                        workspace=None, variant=0):
    """Launch decode attention with a value head size of its own (include/fa2_fwd.h fa2_fwd_kvcache_mla) on the current stream of
    Q's device.  Q (B, H, N_q, d), K (B, H_kv, S_k, d), V (B, H_kv, S_k, d_v) -- V may be a view of K -- or, with block_table, the
    pools (num_blocks, H_kv, page_size, d) / (..., d_v); O (B, H, N_q, d_v), L (B, H, N_q).  The workspace holds
    kvcache_workspace_bytes(B, H, N_q, d_v, num_splits) bytes."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    tb_ptr, tb_st, _, nb, _, mb = _table_args(K, block_table)
    _launch(lib().fa2_fwd_kvcache_mla, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            None if cache_seqlens is None else cache_seqlens.data_ptr(), tb_ptr, tb_st, B, H, K.shape[1], N_q, nb, K.shape[2], mb, d, V.shape[3], int(dtype_enum),
            int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            int(variant), _raw_stream(Q.device.index))


def fa2_fwd_kvcache_mla_fp8(Q, K, V, O, L, cache_seqlens, dtype_enum, kv_dtype_enum, k_descale=None, v_descale=None, block_table=None,
                            causal=False, scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch fa2_fwd_kvcache_mla over an fp8 latent cache (include/fa2_fwd.h fa2_fwd_kvcache_mla_fp8) on the current stream of Q's
    device.  As fa2_fwd_kvcache_mla, with K / V in kv_dtype_enum (an fp8 format; dtype_enum itself: the 16-bit call) and k_descale /
    v_descale as in fa2_fwd_kvcache_fp8: float32 tensors on the device viewed as (B, H_kv), or None for 1."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    tb_ptr, tb_st, _, nb, _, mb = _table_args(K, block_table)
    _launch(lib().fa2_fwd_kvcache_mla_fp8, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            None if cache_seqlens is None else cache_seqlens.data_ptr(), tb_ptr, tb_st, *_descale_args(k_descale, v_descale), B, H,
            K.shape[1], N_q, nb, K.shape[2], mb, d, V.shape[3], int(dtype_enum), int(kv_dtype_enum), int(bool(causal)), float(scale),
            *_window_sides(window), int(num_splits), *_workspace_args(workspace), int(variant), _raw_stream(Q.device.index))


def kvcache_mla_sparse_num_splits(B, H, H_kv, N_q, topk, d, d_v, dtype_enum):
    """What num_splits = 0 resolves to for a sparse latent-cache call of this shape (fa2_kvcache_mla_sparse_num_splits): the splits run
    over the topk slots of the lists."""
    return int(lib().fa2_kvcache_mla_sparse_num_splits(B, H, H_kv, N_q, topk, d, d_v, int(dtype_enum)))


def fa2_fwd_kvcache_mla_sparse(Q, K, V, O, L, indices, cache_seqlens, dtype_enum, kv_dtype_enum, k_descale=None, v_descale=None,
                               block_table=None, scale=1.0, num_splits=0, workspace=None, variant=0):
    """Launch sparse MLA decode (include/fa2_fwd.h fa2_fwd_kvcache_mla_sparse) on the current stream of Q's device.  As
    fa2_fwd_kvcache_mla_fp8 without a mask: indices is an int32 tensor on the device viewed as (B, H_kv, N_q, topk) (expanded views
    are fine: their strides are passed on), entry [b, hk, qi, s] a key position of sequence b, no key outside [0, N_k(b))."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    tb_ptr, tb_st, _, nb, _, mb = _table_args(K, block_table)
    _launch(lib().fa2_fwd_kvcache_mla_sparse, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            None if cache_seqlens is None else cache_seqlens.data_ptr(), indices.data_ptr(), _i64(indices.stride()), indices.shape[3],
            tb_ptr, tb_st, *_descale_args(k_descale, v_descale), B, H, K.shape[1], N_q, nb, K.shape[2], mb, d, V.shape[3],
            int(dtype_enum), int(kv_dtype_enum), float(scale), int(num_splits), *_workspace_args(workspace), int(variant),
            _raw_stream(Q.device.index))


def mla_indexer_workspace_bytes(B, N_q, S_k):
    """Bytes of the contiguous fp32 logits buffer (B, N_q, S_k) of an indexer call (fa2_mla_indexer_workspace_bytes)."""
    return int(lib().fa2_mla_indexer_workspace_bytes(B, N_q, S_k))


def _indexer_args(q_idx, weights, k_idx, k_scale, logits, cache_seqlens, block_table, dtype_enum, k_dtype_enum, causal):
    """The arguments fa2_mla_indexer_logits and fa2_mla_indexer_topk share, in the header's order up to `causal`."""
    B, H_I, N_q, d_I = q_idx.shape
    if block_table is None:
        tb_ptr, tb_st, S_k, nb, ps, mb = None, 0, k_idx.shape[1], 0, 0, 0
    else:
        tb_ptr, tb_st, S_k, nb, ps, mb = block_table.data_ptr(), block_table.stride(0), 0, k_idx.shape[0], k_idx.shape[1], block_table.shape[1]
    return (q_idx.data_ptr(), weights.data_ptr(), k_idx.data_ptr(), _ptr(k_scale), logits.data_ptr(), _i64(q_idx.stride()),
            _i64(weights.stride()), _i64(k_idx.stride()), None if k_scale is None else _i64(k_scale.stride()), _i64(logits.stride()),
            _ptr(cache_seqlens), tb_ptr, tb_st, B, H_I, N_q, S_k, nb, ps, mb, d_I, int(dtype_enum), int(k_dtype_enum), int(bool(causal)))


def fa2_mla_indexer_logits(q_idx, weights, k_idx, k_scale, logits, cache_seqlens, dtype_enum, k_dtype_enum, block_table=None, causal=True,
                           variant=0):
    """Launch the index scores (include/fa2_fwd.h fa2_mla_indexer_logits) on the current stream of q_idx's device: q_idx
    (B, H_I, N_q, d_I), weights fp32 (B, H_I, N_q), k_idx (B, S_k, d_I) or the pool (num_blocks, page_size, d_I) with block_table,
    k_scale fp32 shaped like k_idx's rows or None, logits fp32 (B, N_q, capacity), written for j < n(b, qi).  Any strides."""
    if q_idx.device.type != "cuda":
        raise NotImplementedError("q_idx, weights, k_idx must be on the same CUDA device")
    _launch(lib().fa2_mla_indexer_logits, q_idx,
            *_indexer_args(q_idx, weights, k_idx, k_scale, logits, cache_seqlens, block_table, dtype_enum, k_dtype_enum, causal),
            int(variant), _raw_stream(q_idx.device.index))


def fa2_mla_indexer_topk(q_idx, weights, k_idx, k_scale, logits, indices, cache_seqlens, dtype_enum, k_dtype_enum, block_table=None,
                         causal=True, variant=0):
    """Launch scores and selection on one stream (fa2_mla_indexer_topk): as fa2_mla_indexer_logits, then indices int32
    (B, N_q, topk) from the logits buffer."""
    if q_idx.device.type != "cuda":
        raise NotImplementedError("q_idx, weights, k_idx must be on the same CUDA device")
    _launch(lib().fa2_mla_indexer_topk, q_idx,
            *_indexer_args(q_idx, weights, k_idx, k_scale, logits, cache_seqlens, block_table, dtype_enum, k_dtype_enum, causal),
            indices.shape[2], indices.data_ptr(), _i64(indices.stride()), int(variant), _raw_stream(q_idx.device.index))


def fa2_topk_indices(logits, indices, cache_seqlens, causal=True):
    """Launch the selection alone (fa2_topk_indices) on the current stream of logits' device: logits fp32 (B, N_q, S_k), any
    strides, indices int32 (B, N_q, topk)."""
    if logits.device.type != "cuda":
        raise NotImplementedError("logits must be on a CUDA device")
    B, N_q, S_k = logits.shape
    _launch(lib().fa2_topk_indices, logits, logits.data_ptr(), _i64(logits.stride()), _ptr(cache_seqlens), B, N_q, S_k, indices.shape[2],
            int(bool(causal)), indices.data_ptr(), _i64(indices.stride()), _raw_stream(logits.device.index))


def kvcache_mla_sparse_varlen_num_splits(total_q, H, H_kv, topk, d, d_v, dtype_enum):
    """What num_splits = 0 resolves to for a packed sparse latent-cache call (fa2_kvcache_mla_sparse_varlen_num_splits): the fixed
    call's count with total_q tokens in B * N_q's place."""
    return int(lib().fa2_kvcache_mla_sparse_varlen_num_splits(total_q, H, H_kv, topk, d, d_v, int(dtype_enum)))


def fa2_fwd_kvcache_mla_sparse_varlen(Q, K, V, O, L, indices, cu_q, max_q, cache_seqlens, dtype_enum, kv_dtype_enum, k_descale=None,
                                      v_descale=None, block_table=None, scale=1.0, num_splits=0, workspace=None, variant=0):
    """Launch sparse MLA decode of packed queries (include/fa2_fwd.h fa2_fwd_kvcache_mla_sparse_varlen) on the current stream of Q's
    device.  Q (total_q, H, d), O (total_q, H, d_v), any strides, L (H, total_q) with unit token stride, cu_q int32 (B + 1,) on the
    device; indices an int32 tensor on the device viewed as (total_q, H_kv, topk) (expanded views are fine), entry [t, hk, s] a key
    position of the sequence that owns packed row t.  The cache side is fa2_fwd_kvcache_mla_sparse's.  The workspace holds
    kvcache_varlen_workspace_bytes(total_q, H, d_v, num_splits) bytes."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    total_q, H, d = Q.shape
    _check_packed_l("fa2_fwd_kvcache_mla_sparse_varlen", L, H, total_q)
    tb_ptr, tb_st, _, nb, _, mb = _table_args(K, block_table)
    _launch(lib().fa2_fwd_kvcache_mla_sparse_varlen, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), L.stride(0), cu_q.data_ptr(), _ptr(cache_seqlens),
            indices.data_ptr(), _i64(indices.stride()), indices.shape[2], tb_ptr, tb_st, *_descale_args(k_descale, v_descale),
            cu_q.numel() - 1, H, K.shape[1], total_q, int(max_q), nb, K.shape[2], mb, d, V.shape[3], int(dtype_enum), int(kv_dtype_enum),
            float(scale), int(num_splits), *_workspace_args(workspace), int(variant), _raw_stream(Q.device.index))


def mla_indexer_varlen_workspace_bytes(total_q, S_k):
    """Bytes of the contiguous fp32 logits buffer (total_q, S_k) of a packed indexer call (fa2_mla_indexer_varlen_workspace_bytes)."""
    return int(lib().fa2_mla_indexer_varlen_workspace_bytes(total_q, S_k))


def _indexer_varlen_args(q_idx, weights, k_idx, k_scale, logits, cu_q, max_q, cache_seqlens, block_table, dtype_enum, k_dtype_enum, causal):
    """The arguments fa2_mla_indexer_logits_varlen and fa2_mla_indexer_topk_varlen share, in the header's order up to `causal`."""
    total_q, H_I, d_I = q_idx.shape
    if block_table is None:
        tb_ptr, tb_st, S_k, nb, ps, mb = None, 0, k_idx.shape[1], 0, 0, 0
    else:
        tb_ptr, tb_st, S_k, nb, ps, mb = block_table.data_ptr(), block_table.stride(0), 0, k_idx.shape[0], k_idx.shape[1], block_table.shape[1]
    return (q_idx.data_ptr(), weights.data_ptr(), k_idx.data_ptr(), _ptr(k_scale), logits.data_ptr(), _i64(q_idx.stride()),
            _i64(weights.stride()), _i64(k_idx.stride()), None if k_scale is None else _i64(k_scale.stride()), _i64(logits.stride()),
            cu_q.data_ptr(), _ptr(cache_seqlens), tb_ptr, tb_st, cu_q.numel() - 1, H_I, total_q, int(max_q), S_k, nb, ps, mb, d_I,
            int(dtype_enum), int(k_dtype_enum), int(bool(causal)))


def fa2_mla_indexer_logits_varlen(q_idx, weights, k_idx, k_scale, logits, cu_q, max_q, cache_seqlens, dtype_enum, k_dtype_enum,
                                  block_table=None, causal=True, variant=0):
    """Launch the index scores of packed queries (include/fa2_fwd.h fa2_mla_indexer_logits_varlen) on the current stream of q_idx's
    device: q_idx (total_q, H_I, d_I), weights fp32 (total_q, H_I), logits fp32 (total_q, capacity), cu_q int32 (B + 1,) on the
    device; the key side as fa2_mla_indexer_logits.  Any strides."""
    if q_idx.device.type != "cuda":
        raise NotImplementedError("q_idx, weights, k_idx must be on the same CUDA device")
    _launch(lib().fa2_mla_indexer_logits_varlen, q_idx,
            *_indexer_varlen_args(q_idx, weights, k_idx, k_scale, logits, cu_q, max_q, cache_seqlens, block_table, dtype_enum, k_dtype_enum,
                                  causal),
            int(variant), _raw_stream(q_idx.device.index))


def fa2_mla_indexer_topk_varlen(q_idx, weights, k_idx, k_scale, logits, indices, cu_q, max_q, cache_seqlens, dtype_enum, k_dtype_enum,
                                block_table=None, causal=True, variant=0):
    """Launch scores and selection of packed queries on one stream (fa2_mla_indexer_topk_varlen): as fa2_mla_indexer_logits_varlen,
    then indices int32 (total_q, topk) from the logits buffer."""
    if q_idx.device.type != "cuda":
        raise NotImplementedError("q_idx, weights, k_idx must be on the same CUDA device")
    _launch(lib().fa2_mla_indexer_topk_varlen, q_idx,
            *_indexer_varlen_args(q_idx, weights, k_idx, k_scale, logits, cu_q, max_q, cache_seqlens, block_table, dtype_enum, k_dtype_enum,
                                  causal),
            indices.shape[1], indices.data_ptr(), _i64(indices.stride()), int(variant), _raw_stream(q_idx.device.index))


def fa2_topk_indices_varlen(logits, indices, cu_q, max_q, cache_seqlens, causal=True):
    """Launch the packed selection alone (fa2_topk_indices_varlen) on the current stream of logits' device: logits fp32
    (total_q, S_k), any strides, indices int32 (total_q, topk)."""
    if logits.device.type != "cuda":
        raise NotImplementedError("logits must be on a CUDA device")
    total_q, S_k = logits.shape
    _launch(lib().fa2_topk_indices_varlen, logits, logits.data_ptr(), _i64(logits.stride()), cu_q.data_ptr(), _ptr(cache_seqlens),
            cu_q.numel() - 1, total_q, int(max_q), S_k, indices.shape[1], int(bool(causal)), indices.data_ptr(), _i64(indices.stride()),
            _raw_stream(logits.device.index))


def _append_args(K, k_new, block_table, k_descale, v_descale, rotary_cos, rotary_sin):
    """The pieces both append launchers pass alike: (table pointer, table stride, descale pointers and strides, rotary pointers,
    row strides, S_rot, rotary_dim, S_k, num_blocks, page_size, max_blocks)."""
    tb_ptr, tb_st, S_k, nb, ps, mb = _table_args(K, block_table)
    cos_st, S_rot, rd = (0, 0, 0) if rotary_cos is None else (rotary_cos.stride(0), rotary_cos.shape[0], 2 * rotary_cos.shape[1])
    sin_st = 0 if rotary_sin is None else rotary_sin.stride(0)
    return (tb_ptr, tb_st, *_descale_args(k_descale, v_descale), _ptr(rotary_cos), _ptr(rotary_sin), cos_st, sin_st, S_rot, rd, S_k, nb,
            ps, mb)


def fa2_kvcache_append(K, V, k_new, v_new, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum, block_table=None, k_descale=None,
                       v_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, Q=None, q_rot=None,
                       q_pos_per_row=False):
    """Launch the cache append (include/fa2_fwd.h fa2_kvcache_append) on the current stream of k_new's device: k_new / v_new
    (B, H_kv, N_new, d), any strides, go into the cache K / V (B, H_kv, S_k, d), or the pool (num_blocks, H_kv, page_size, d) with
    block_table, in place; seqlens_out, an int32 (B,) tensor that is not cache_seqlens, receives the new lengths.  rotary_cos /
    rotary_sin (S_rot, rotary_dim / 2) in k_new's dtype with unit last stride; Q (B, H, N_q, d) with them is rotated into the
    contiguous q_rot.  Descales as in fa2_fwd_kvcache_fp8."""
    if k_new.device.type != "cuda":
        raise NotImplementedError("K_cache, V_cache, k_new, v_new must be on the same CUDA device")
    B, H_kv, N_new, d = k_new.shape
    tb_ptr, tb_st, kd_ptr, vd_ptr, kd_st, vd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _append_args(K, k_new, block_table, k_descale, v_descale, rotary_cos, rotary_sin)
    q_st, H, N_q = (None, 0, 0) if Q is None else (_i64(Q.stride()), Q.shape[1], Q.shape[2])
    _launch(lib().fa2_kvcache_append, k_new,
            K.data_ptr(), V.data_ptr(), _i64(K.stride()), _i64(V.stride()), tb_ptr, tb_st, k_new.data_ptr(), v_new.data_ptr(),
            _i64(k_new.stride()), _i64(v_new.stride()), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), kd_ptr, vd_ptr, kd_st, vd_st,
            cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, int(bool(rotary_interleaved)), _ptr(Q), _ptr(q_rot), q_st, H, N_q,
            int(bool(q_pos_per_row)), B, H_kv, N_new, S_k, nb, ps, mb, d, int(dtype_enum), int(kv_dtype_enum),
            _raw_stream(k_new.device.index))


def fa2_fwd_kvcache_append(Q, K, V, O, L, k_new, v_new, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum, block_table=None,
                           k_descale=None, v_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None,
                           causal=False, scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch the fused decode step (include/fa2_fwd.h fa2_fwd_kvcache_append) on the current stream of Q's device: the append
    above, then the decode attention over the updated cache with seqlens_out as its lengths and, with rotary tables, q_rot (a
    contiguous (B, H, N_q, d) tensor in Q's dtype) as its Q.  The other arguments are fa2_fwd_kvcache_paged's."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    tb_ptr, tb_st, kd_ptr, vd_ptr, kd_st, vd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _append_args(K, k_new, block_table, k_descale, v_descale, rotary_cos, rotary_sin)
    _launch(lib().fa2_fwd_kvcache_append, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), _i64((L.stride(0), L.stride(1))),
            cache_seqlens.data_ptr(), seqlens_out.data_ptr(), tb_ptr, tb_st, kd_ptr, vd_ptr, kd_st, vd_st, k_new.data_ptr(),
            v_new.data_ptr(), _i64(k_new.stride()), _i64(v_new.stride()), cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd,
            int(bool(rotary_interleaved)), _ptr(q_rot), B, H, K.shape[1], N_q, k_new.shape[2], S_k, nb, ps, mb, d, int(dtype_enum),
            int(kv_dtype_enum), int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            int(variant), _raw_stream(Q.device.index))


def kvcache_varlen_num_splits(B, H, H_kv, total_q, max_seqlen_q, S_k, d, dtype_enum):
    """What num_splits = 0 resolves to for a packed-query call of this shape (fa2_kvcache_varlen_num_splits)."""
    return int(lib().fa2_kvcache_varlen_num_splits(B, H, H_kv, total_q, max_seqlen_q, S_k, d, int(dtype_enum)))


def kvcache_varlen_workspace_bytes(total_q, H, d, num_splits):
    """Bytes of fp32 workspace a packed-query call with this num_splits needs (fa2_kvcache_varlen_workspace_bytes)."""
    return int(lib().fa2_kvcache_varlen_workspace_bytes(total_q, H, d, num_splits))


def fa2_fwd_kvcache_varlen(Q, K, V, O, L, cu_q, max_q, cache_seqlens, dtype_enum, kv_dtype_enum, block_table=None, k_descale=None,
                           v_descale=None, causal=False, scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch attention of packed queries over the KV cache (include/fa2_fwd.h fa2_fwd_kvcache_varlen) on the current stream of Q's
    device.  Q, O (total_q, H, d) with any strides, L (H, total_q) with unit token stride, cu_q int32 (B + 1,) on the device; K / V
    the cache (B, H_kv, S_k, d) or, with block_table, the pool (num_blocks, H_kv, page_size, d); the rest as fa2_fwd_kvcache_paged."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    total_q, H, d = Q.shape
    if L.dim() != 2 or L.shape != (H, total_q) or (total_q > 1 and L.stride(1) != 1):  # the ABI takes the head stride alone
        raise ValueError(f"fa2_fwd_kvcache_varlen: L must be (H, total_q) = ({H}, {total_q}) with unit token stride, got "
                         f"{tuple(L.shape)} with strides {tuple(L.stride())}")
    tb_ptr, tb_st, S_k, nb, ps, mb = _table_args(K, block_table)
    _launch(lib().fa2_fwd_kvcache_varlen, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), L.stride(0),
            cu_q.data_ptr(), None if cache_seqlens is None else cache_seqlens.data_ptr(), tb_ptr, tb_st, *_descale_args(k_descale, v_descale),
            cu_q.numel() - 1, H, K.shape[1], total_q, int(max_q), S_k, nb, ps, mb, d, int(dtype_enum), int(kv_dtype_enum),
            int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            int(variant), _raw_stream(Q.device.index))


def fa2_kvcache_append_varlen(K, V, k_new, v_new, cu_new, max_new, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum, block_table=None,
                              k_descale=None, v_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, Q=None,
                              q_rot=None, q_pos_per_row=False):
    """Launch the packed cache append (include/fa2_fwd.h fa2_kvcache_append_varlen) on the current stream of k_new's device: k_new /
    v_new packed (total_new, H_kv, d), any strides, over cu_new, an int32 (B + 1,) tensor on the device, go into the cache K / V
    (B, H_kv, S_k, d), or the pool with block_table, in place; seqlens_out, an int32 (B,) tensor that is not cache_seqlens, receives
    the new lengths.  Q packed (total_new, H, d) with rotary tables is rotated into the contiguous q_rot.  The rest as
    fa2_kvcache_append."""
    if k_new.device.type != "cuda":
        raise NotImplementedError("K_cache, V_cache, k_new, v_new must be on the same CUDA device")
    total_new, H_kv, d = k_new.shape
    tb_ptr, tb_st, kd_ptr, vd_ptr, kd_st, vd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _append_args(K, k_new, block_table, k_descale, v_descale, rotary_cos, rotary_sin)
    q_st, H = (None, 0) if Q is None else (_i64(Q.stride()), Q.shape[1])
    _launch(lib().fa2_kvcache_append_varlen, k_new,
            K.data_ptr(), V.data_ptr(), _i64(K.stride()), _i64(V.stride()), tb_ptr, tb_st, k_new.data_ptr(), v_new.data_ptr(),
            _i64(k_new.stride()), _i64(v_new.stride()), cu_new.data_ptr(), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), kd_ptr,
            vd_ptr, kd_st, vd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, int(bool(rotary_interleaved)), _ptr(Q), _ptr(q_rot),
            q_st, H, int(bool(q_pos_per_row)), cu_new.numel() - 1, H_kv, total_new, int(max_new), S_k, nb, ps, mb, d, int(dtype_enum),
            int(kv_dtype_enum), _raw_stream(k_new.device.index))


def fa2_fwd_kvcache_varlen_append(Q, K, V, O, L, k_new, v_new, cu_q, max_q, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum,
                                  block_table=None, k_descale=None, v_descale=None, rotary_cos=None, rotary_sin=None,
                                  rotary_interleaved=False, q_rot=None, causal=False, scale=1.0, window=None, num_splits=0,
                                  workspace=None, variant=0):
    """Launch the fused ragged step (include/fa2_fwd.h fa2_fwd_kvcache_varlen_append) on the current stream of Q's device: the packed
    append above with cu_q as its offsets (k_new, v_new (total_q, H_kv, d)), then fa2_fwd_kvcache_varlen over the updated cache with
    seqlens_out as its lengths and, with rotary tables, q_rot (a contiguous (total_q, H, d) tensor in Q's dtype) as its Q."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    total_q, H, d = Q.shape
    if L.dim() != 2 or L.shape != (H, total_q) or (total_q > 1 and L.stride(1) != 1):  # the ABI takes the head stride alone
        raise ValueError(f"fa2_fwd_kvcache_varlen_append: L must be (H, total_q) = ({H}, {total_q}) with unit token stride, got "
                         f"{tuple(L.shape)} with strides {tuple(L.stride())}")
    tb_ptr, tb_st, kd_ptr, vd_ptr, kd_st, vd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _append_args(K, k_new, block_table, k_descale, v_descale, rotary_cos, rotary_sin)
    _launch(lib().fa2_fwd_kvcache_varlen_append, Q,
            Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(),
            _i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O.stride()), L.stride(0),
            cu_q.data_ptr(), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), tb_ptr, tb_st, kd_ptr, vd_ptr, kd_st, vd_st,
            k_new.data_ptr(), v_new.data_ptr(), _i64(k_new.stride()), _i64(v_new.stride()), cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd,
            int(bool(rotary_interleaved)), _ptr(q_rot), cu_q.numel() - 1, H, K.shape[1], total_q, int(max_q), S_k, nb, ps, mb, d,
            int(dtype_enum), int(kv_dtype_enum), int(bool(causal)), float(scale), *_window_sides(window), int(num_splits),
            *_workspace_args(workspace), int(variant), _raw_stream(Q.device.index))


def _mla_append_args(KV, block_table, kv_descale, rotary_cos, rotary_sin):
    """_append_args for the latent cache and its one descale: (table pointer, table stride, descale pointer, descale strides, rotary
    pointers, row strides, S_rot, rotary_dim, S_k, num_blocks, page_size, max_blocks)."""
    tb_ptr, tb_st, kd_ptr, _, kd_st, _, *rest = _append_args(KV, None, block_table, kv_descale, None, rotary_cos, rotary_sin)
    return (tb_ptr, tb_st, kd_ptr, kd_st, *rest)


def fa2_kvcache_mla_append(KV, c_new, pe_new, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum, block_table=None, kv_descale=None,
                           rotary_cos=None, rotary_sin=None, rotary_interleaved=False, Q=None, q_rot=None, q_pos_per_row=False):
    """Launch the latent-cache append (include/fa2_fwd.h fa2_kvcache_mla_append) on the current stream of c_new's device: c_new
    (B, H_kv, N_new, d_v) and pe_new (B, H_kv, N_new, d - d_v), any strides, become the columns [0, d_v) and [d_v, d) of new rows of
    KV (B, H_kv, S_k, d), or the pool (num_blocks, H_kv, page_size, d) with block_table, in place; seqlens_out, an int32 (B,) tensor
    that is not cache_seqlens, receives the new lengths.  rotary_cos / rotary_sin (S_rot, rotary_dim / 2) rotate the columns
    [d_v, d_v + rotary_dim), of Q (B, H, N_q, d) too, which goes to the contiguous q_rot.  kv_descale as k_descale in
    fa2_kvcache_append."""
    if c_new.device.type != "cuda":
        raise NotImplementedError("KV_cache, c_new, pe_new must be on the same CUDA device")
    B, H_kv, N_new, d_v = c_new.shape
    tb_ptr, tb_st, kd_ptr, kd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _mla_append_args(KV, block_table, kv_descale, rotary_cos, rotary_sin)
    q_st, H, N_q = (None, 0, 0) if Q is None else (_i64(Q.stride()), Q.shape[1], Q.shape[2])
    _launch(lib().fa2_kvcache_mla_append, c_new,
            KV.data_ptr(), _i64(KV.stride()), tb_ptr, tb_st, c_new.data_ptr(), pe_new.data_ptr(), _i64(c_new.stride()),
            _i64(pe_new.stride()), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), kd_ptr, kd_st, cos_ptr, sin_ptr, cos_st, sin_st,
            S_rot, rd, int(bool(rotary_interleaved)), _ptr(Q), _ptr(q_rot), q_st, H, N_q, int(bool(q_pos_per_row)), B, H_kv, N_new,
            S_k, nb, ps, mb, KV.shape[3], d_v, int(dtype_enum), int(kv_dtype_enum), _raw_stream(c_new.device.index))


def fa2_kvcache_mla_append_varlen(KV, c_new, pe_new, cu_new, max_new, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum,
                                  block_table=None, kv_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, Q=None,
                                  q_rot=None, q_pos_per_row=False):
    """Launch the packed latent-cache append (include/fa2_fwd.h fa2_kvcache_mla_append_varlen) on the current stream of c_new's
    device: fa2_kvcache_mla_append with c_new (total_new, H_kv, d_v), pe_new (total_new, H_kv, d - d_v) and Q, q_rot (total_new, H, d)
    packed over cu_new, an int32 (B + 1,) tensor on the device."""
    if c_new.device.type != "cuda":
        raise NotImplementedError("KV_cache, c_new, pe_new must be on the same CUDA device")
    total_new, H_kv, d_v = c_new.shape
    tb_ptr, tb_st, kd_ptr, kd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _mla_append_args(KV, block_table, kv_descale, rotary_cos, rotary_sin)
    q_st, H = (None, 0) if Q is None else (_i64(Q.stride()), Q.shape[1])
    _launch(lib().fa2_kvcache_mla_append_varlen, c_new,
            KV.data_ptr(), _i64(KV.stride()), tb_ptr, tb_st, c_new.data_ptr(), pe_new.data_ptr(), _i64(c_new.stride()),
            _i64(pe_new.stride()), cu_new.data_ptr(), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), kd_ptr, kd_st, cos_ptr, sin_ptr,
            cos_st, sin_st, S_rot, rd, int(bool(rotary_interleaved)), _ptr(Q), _ptr(q_rot), q_st, H, int(bool(q_pos_per_row)),
            cu_new.numel() - 1, H_kv, total_new, int(max_new), S_k, nb, ps, mb, KV.shape[3], d_v, int(dtype_enum), int(kv_dtype_enum),
            _raw_stream(c_new.device.index))


def fa2_fwd_kvcache_mla_append(Q, KV, O, L, c_new, pe_new, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum, block_table=None,
                               kv_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False, q_rot=None, causal=False,
                               scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch the fused MLA decode step (include/fa2_fwd.h fa2_fwd_kvcache_mla_append) on the current stream of Q's device: the
    append above, then the latent-cache decode over the updated KV with seqlens_out as its lengths and, with rotary tables, q_rot (a
    contiguous (B, H, N_q, d) tensor in Q's dtype) as its Q.  O (B, H, N_q, d_v), L (B, H, N_q); the workspace holds
    kvcache_workspace_bytes(B, H, N_q, d_v, num_splits) bytes."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    B, H, N_q, d = Q.shape
    tb_ptr, tb_st, kd_ptr, kd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _mla_append_args(KV, block_table, kv_descale, rotary_cos, rotary_sin)
    _launch(lib().fa2_fwd_kvcache_mla_append, Q,
            Q.data_ptr(), KV.data_ptr(), O.data_ptr(), L.data_ptr(), _i64(Q.stride()), _i64(KV.stride()), _i64(O.stride()),
            _i64((L.stride(0), L.stride(1))), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), tb_ptr, tb_st, kd_ptr, kd_st,
            c_new.data_ptr(), pe_new.data_ptr(), _i64(c_new.stride()), _i64(pe_new.stride()), cos_ptr, sin_ptr, cos_st, sin_st, S_rot,
            rd, int(bool(rotary_interleaved)), _ptr(q_rot), B, H, KV.shape[1], N_q, c_new.shape[2], S_k, nb, ps, mb, d, c_new.shape[3],
            int(dtype_enum), int(kv_dtype_enum), int(bool(causal)), float(scale), *_window_sides(window), int(num_splits),
            *_workspace_args(workspace), int(variant), _raw_stream(Q.device.index))


def kvcache_mla_varlen_num_splits(B, H, H_kv, total_q, max_seqlen_q, S_k, d, d_v, dtype_enum):
    """What num_splits = 0 resolves to for a packed-query call over the latent cache (fa2_kvcache_mla_varlen_num_splits)."""
    return int(lib().fa2_kvcache_mla_varlen_num_splits(B, H, H_kv, total_q, max_seqlen_q, S_k, d, d_v, int(dtype_enum)))


def _check_packed_l(who, L, H, total_q):
    if L.dim() != 2 or L.shape != (H, total_q) or (total_q > 1 and L.stride(1) != 1):  # the ABI takes the head stride alone
        raise ValueError(f"{who}: L must be (H, total_q) = ({H}, {total_q}) with unit token stride, got {tuple(L.shape)} with strides "
                         f"{tuple(L.stride())}")


def fa2_fwd_kvcache_mla_varlen(Q, KV, O, L, cu_q, max_q, cache_seqlens, dtype_enum, kv_dtype_enum, d_v, block_table=None, kv_descale=None,
                               causal=False, scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch attention of packed queries over the latent cache (include/fa2_fwd.h fa2_fwd_kvcache_mla_varlen) on the current stream
    of Q's device.  Q (total_q, H, d), O (total_q, H, d_v), any strides, L (H, total_q) with unit token stride, cu_q int32 (B + 1,) on
    the device; KV the latent cache (B, H_kv, S_k, d) or, with block_table, the pool (num_blocks, H_kv, page_size, d); kv_descale a
    float32 tensor viewed as (B, H_kv), or None for 1.  The workspace holds kvcache_varlen_workspace_bytes(total_q, H, d_v,
    num_splits) bytes."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    total_q, H, d = Q.shape
    _check_packed_l("fa2_fwd_kvcache_mla_varlen", L, H, total_q)
    tb_ptr, tb_st, S_k, nb, ps, mb = _table_args(KV, block_table)
    kd_ptr, _, kd_st, _ = _descale_args(kv_descale, None)
    _launch(lib().fa2_fwd_kvcache_mla_varlen, Q,
            Q.data_ptr(), KV.data_ptr(), O.data_ptr(), L.data_ptr(), _i64(Q.stride()), _i64(KV.stride()), _i64(O.stride()), L.stride(0),
            cu_q.data_ptr(), None if cache_seqlens is None else cache_seqlens.data_ptr(), tb_ptr, tb_st, kd_ptr, kd_st,
            cu_q.numel() - 1, H, KV.shape[1], total_q, int(max_q), S_k, nb, ps, mb, d, int(d_v), int(dtype_enum), int(kv_dtype_enum),
            int(bool(causal)), float(scale), *_window_sides(window), int(num_splits), *_workspace_args(workspace),
            int(variant), _raw_stream(Q.device.index))


def fa2_fwd_kvcache_mla_varlen_append(Q, KV, O, L, c_new, pe_new, cu_q, max_q, cache_seqlens, seqlens_out, dtype_enum, kv_dtype_enum,
                                      block_table=None, kv_descale=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False,
                                      q_rot=None, causal=False, scale=1.0, window=None, num_splits=0, workspace=None, variant=0):
    """Launch the fused ragged MLA step (include/fa2_fwd.h fa2_fwd_kvcache_mla_varlen_append) on the current stream of Q's device:
    fa2_kvcache_mla_append_varlen with cu_q as its offsets (c_new (total_q, H_kv, d_v), pe_new (total_q, H_kv, d - d_v)), then
    fa2_fwd_kvcache_mla_varlen over the updated KV with seqlens_out as its lengths and, with rotary tables, q_rot (a contiguous
    (total_q, H, d) tensor in Q's dtype) as its Q."""
    if Q.device.type != "cuda":
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    total_q, H, d = Q.shape
    _check_packed_l("fa2_fwd_kvcache_mla_varlen_append", L, H, total_q)
    tb_ptr, tb_st, kd_ptr, kd_st, cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd, S_k, nb, ps, mb = \
        _mla_append_args(KV, block_table, kv_descale, rotary_cos, rotary_sin)
    _launch(lib().fa2_fwd_kvcache_mla_varlen_append, Q,
            Q.data_ptr(), KV.data_ptr(), O.data_ptr(), L.data_ptr(), _i64(Q.stride()), _i64(KV.stride()), _i64(O.stride()), L.stride(0),
            cu_q.data_ptr(), cache_seqlens.data_ptr(), seqlens_out.data_ptr(), tb_ptr, tb_st, kd_ptr, kd_st, c_new.data_ptr(),
            pe_new.data_ptr(), _i64(c_new.stride()), _i64(pe_new.stride()), cos_ptr, sin_ptr, cos_st, sin_st, S_rot, rd,
            int(bool(rotary_interleaved)), _ptr(q_rot), cu_q.numel() - 1, H, KV.shape[1], total_q, int(max_q), S_k, nb, ps, mb, d,
            c_new.shape[2], int(dtype_enum), int(kv_dtype_enum), int(bool(causal)), float(scale), *_window_sides(window),
            int(num_splits), *_workspace_args(workspace), int(variant), _raw_stream(Q.device.index))
