"""Dense MLA decode over the tile-scaled fp8 cache (flash_attention_mla_decode_forward(..., kv_format="fp8_ds")) on the GPU.  The result
is DEFINED as the 16-bit call's on dequantize_mla_cache_ds(KV8, T), bit for bit at the same variant and num_splits: no tolerance."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import check_forward, lens_of
from test_decode_mla_gpu import reference
from test_decode_mla_sparse_ds_gpu import make_ds
from test_decode_mla_sparse_gpu import SCALE, paged, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16 = torch.float16, torch.bfloat16
S_K, LENS = 200, [0, 1, 63, 64, 65, 129, 200]  # an empty sequence, a tile edge from both sides, a split edge inside a tile, the capacity
MASKS = [dict(), dict(causal=True), dict(window=(70, 0))]
ids = lambda x: str(x).replace("torch.", "")
dense = fa.flash_attention_mla_decode_forward


@functools.lru_cache(maxsize=None)
def case(dtype, H, N_q):
    """Q, the fp8_ds cache (the sparse fp8_ds tests' magnitudes) and the rows it stands for"""
    Q, KV8 = make_ds(len(LENS), H, 1, N_q, S_K, dtype, 5 * H + N_q)
    return Q, KV8, fa.dequantize_mla_cache_ds(KV8, dtype)


@pytest.mark.parametrize("mask", MASKS, ids=ids)
@pytest.mark.parametrize("H,N_q", [(16, 1), (16, 2), (128, 1), (128, 2)])
@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_equals_the_16_bit_call_on_the_dequantised_cache_bit_for_bit(dtype, variant, H, N_q, mask):
    Q, KV8, D = case(dtype, H, N_q)
    for n in (1, 3):
        kw = dict(scale=SCALE, num_splits=n, variant=variant, **mask)
        O, L = dense(Q, KV8, lens_of(LENS), DEV, kv_format="fp8_ds", **kw)
        O16, L16 = dense(Q, D, lens_of(LENS), DEV, **kw)
        assert O.shape == O16.shape and not torch.isnan(O.float()).any() and same_bits(O, O16) and same_bits(L, L16), n


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_matrix_form_against_the_fp64_softmax_over_the_dequantised_rows(dtype):
    Q, KV8, D = case(dtype, 128, 2)
    O_ref, L_ref = reference(Q, D, D[..., :512], LENS, True, SCALE, None)
    O, L = dense(Q, KV8, lens_of(LENS), DEV, causal=True, scale=SCALE, num_splits=3, variant="mla16", kv_format="fp8_ds")
    check_forward(O, L, O_ref, L_ref, dtype, dtype)


def poisoned(KV8):
    """every row behind cache_seqlens[b] filled with 0xff: NaN e4m3 bytes, NaN scales, NaN rotary columns"""
    cache = KV8.clone()
    for b, nk in enumerate(LENS):
        cache[b, :, nk:] = 0xff
    return cache


@pytest.mark.parametrize("page,variant", [(64, "mla16"), (64, "generic"), (16, "auto"), (16, "generic")])
def test_paged_and_poisoned_equals_contiguous_bit_for_bit(page, variant):
    """a permuted block table, spare pages and every row no sequence holds in 0xff bytes"""
    Q, KV8, _ = case(BF16, 16, 2)
    pool, table = paged(poisoned(KV8), page, 33, fill=255.0)
    assert int((pool == 255).all(-1).all(-1).all(-1).sum()) >= 3
    for n in (1, 3):
        kw = dict(causal=True, scale=SCALE, num_splits=n, kv_format="fp8_ds")
        O, L = dense(Q, KV8, lens_of(LENS), DEV, variant=variant if page == 64 else "generic", **kw)  # (page 16: auto is the VALU form)
        Op, Lp = dense(Q, pool, lens_of(LENS), DEV, block_table=table, variant=variant, **kw)
        assert not torch.isnan(Op.float()).any() and same_bits(O, Op) and same_bits(L, Lp), n


@pytest.mark.parametrize("variant", ["mla16", "generic"])
def test_rows_behind_the_lengths_and_the_workspace_are_never_read(variant):
    Q, KV8, _ = case(F16, 128, 2)
    B, H, N_q = Q.shape[:3]
    for n in (1, 3):
        results = []
        for cache in (KV8, poisoned(KV8)):
            O, L = torch.empty(B, H, N_q, 512, dtype=F16, device=DEV), torch.empty(B, H, N_q, dtype=F16, device=DEV)
            ws = torch.full((max(_lib.kvcache_workspace_bytes(B, H, N_q, 512, n) // 4, 1),), math.nan, device=DEV)
            _lib.fa2_fwd_kvcache_mla_ds(Q, cache, O, L, lens_of(LENS), convert_triton_dtype(F16), causal=True, scale=SCALE, num_splits=n,
                                        workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
            results.append((O, L))
        assert not torch.isnan(results[0][0].float()).any()
        assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1]), n


def test_a_misaligned_view_runs_on_the_valu_form_and_the_forced_matrix_form_refuses_it():
    Q, KV8, _ = case(BF16, 16, 2)
    wide = torch.zeros(*KV8.shape[:3], 660, dtype=torch.uint8, device=DEV)
    view = wide[..., 4:]  # base + 4 bytes, a row stride of 660
    view.copy_(KV8)
    kw = dict(scale=SCALE, num_splits=3, kv_format="fp8_ds")
    with pytest.raises(TypeError, match="16 bytes"):  # FA2_ERR_UNSUPPORTED
        dense(Q, view, lens_of(LENS), DEV, variant="mla16", **kw)
    Og, Lg = dense(Q, KV8, lens_of(LENS), DEV, variant="generic", **kw)
    for variant in ("auto", "generic"):
        O, L = dense(Q, view, lens_of(LENS), DEV, variant=variant, **kw)
        assert same_bits(O, Og) and same_bits(L, Lg), variant
