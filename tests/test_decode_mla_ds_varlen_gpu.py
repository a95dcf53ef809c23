"""Packed dense MLA decode over the tile-scaled fp8 cache (flash_attention_mla_varlen_decode_forward(..., kv_format="fp8_ds")) on the
GPU: bit for bit the 16-bit packed call on the dequantised cache, and each sequence's rows the fixed call's on that sequence alone."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import lens_of
from test_decode_mla_sparse_ds_gpu import make_ds
from test_decode_mla_sparse_gpu import SCALE, same_bits
from test_decode_mla_varlen_gpu import cu_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16 = torch.float16, torch.bfloat16
H, S_K = 16, 200
N_Q, N_K = [0, 1, 3, 70], [65, 0, 129, 200]  # no query, no key, a few rows, 1,120 rows across 64-row tiles
TOTAL, SPARE = sum(N_Q), 2                    # ... and two packed rows behind the last sequence that no sequence owns
MASKS = [dict(), dict(causal=True), dict(window=(70, 0))]
ids = lambda x: str(x).replace("torch.", "")
packed = fa.flash_attention_mla_varlen_decode_forward


@functools.lru_cache(maxsize=None)
def case(dtype):
    Q, KV8 = make_ds(len(N_Q), H, 1, TOTAL + SPARE, S_K, dtype, 17)
    return Q[0].transpose(0, 1).contiguous(), KV8, fa.dequantize_mla_cache_ds(KV8, dtype)  # Q packed (TOTAL + SPARE, H, 576)


@pytest.mark.parametrize("mask", MASKS, ids=ids)
@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_equals_the_16_bit_packed_call_and_the_fixed_call_on_each_sequence_alone(dtype, variant, mask):
    Q, KV8, D = case(dtype)
    for n in (1, 3):
        kw = dict(scale=SCALE, num_splits=n, variant=variant, **mask)
        O, L = packed(Q[:TOTAL], KV8, cu_of(N_Q), max(N_Q), lens_of(N_K), DEV, kv_format="fp8_ds", **kw)
        O16, L16 = packed(Q[:TOTAL], D, cu_of(N_Q), max(N_Q), lens_of(N_K), DEV, **kw)
        assert O.shape == (TOTAL, H, 512) and L.shape == (H, TOTAL) and not torch.isnan(O.float()).any()
        assert same_bits(O, O16) and same_bits(L, L16), n
        start = 0
        for b, (nq, nk) in enumerate(zip(N_Q, N_K)):
            if nq:
                Ob, Lb = fa.flash_attention_mla_decode_forward(Q[start:start + nq].transpose(0, 1)[None], KV8[b:b + 1], lens_of([nk]), DEV,
                                                               kv_format="fp8_ds", **kw)
                assert same_bits(Ob[0].transpose(0, 1), O[start:start + nq]) and same_bits(Lb[0], L[:, start:start + nq]), (n, b)
            start += nq


@pytest.mark.parametrize("variant", ["mla16", "generic"])
def test_max_seqlen_q_below_the_longest_count_and_rows_no_sequence_owns(variant):
    """max_seqlen_q = 64 under a count of 70: the sequence owns its first 64 rows; its other six and the spare rows keep their canary"""
    Q, KV8, _ = case(BF16)
    kw = dict(scale=SCALE, num_splits=3, variant=variant)
    O_full, L_full = packed(Q[:TOTAL], KV8, cu_of(N_Q), max(N_Q), lens_of(N_K), DEV, kv_format="fp8_ds", **kw)
    O = torch.full((TOTAL + SPARE, H, 512), 7.0, dtype=BF16, device=DEV)
    L = torch.full((H, TOTAL + SPARE), 7.0, dtype=BF16, device=DEV)
    ws = torch.empty(_lib.kvcache_varlen_workspace_bytes(TOTAL + SPARE, H, 512, 3) // 4, device=DEV)
    _lib.fa2_fwd_kvcache_mla_varlen_ds(Q, KV8, O, L, cu_of(N_Q), 64, lens_of(N_K), convert_triton_dtype(BF16), scale=SCALE, num_splits=3,
                                       workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
    owned = TOTAL - 6
    assert same_bits(O[:owned], O_full[:owned]) and same_bits(L[:, :owned], L_full[:, :owned])  # (no mask: a row does not see the count)
    assert (O[owned:] == 7.0).all() and (L[:, owned:] == 7.0).all()
