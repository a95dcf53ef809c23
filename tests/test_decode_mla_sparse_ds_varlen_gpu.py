"""Packed sparse MLA decode over the tile-scaled fp8 cache (kv_format="fp8_ds") on the GPU: the packed call equals the packed 16-bit
call on the dequantised cache bit for bit, and sequence b's rows equal the fixed kv_format call on that sequence alone."""
import pytest
import torch

import flash_attention_dlrs_amd as fa
from test_decode_gpu import lens_of
from test_decode_mla_sparse_ds_gpu import make_ds
from test_decode_mla_sparse_gpu import SCALE, same_bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CU = [0, 1, 1, 4, 12]  # sequence 1 has no query; packed row 12 lies beyond the last offset: no sequence owns it
LENS, S_K, TOTAL, MAX_Q = [65, 320, 0, 300], 320, 13, 8


@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("H,H_kv,topk,n", [(40, 1, 130, 3), (32, 2, 65, 1)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_packed_equals_the_16_bit_packed_call_and_the_fixed_call_per_sequence(dtype, H, H_kv, topk, n, variant):
    B = len(LENS)
    Qf, KV8 = make_ds(B, H, H_kv, TOTAL, S_K, dtype, 5 + H)
    Q = Qf[0].transpose(0, 1).contiguous()  # (total_q, H, 576)
    g = torch.Generator().manual_seed(topk)
    idx = torch.randint(0, S_K, (TOTAL, H_kv, topk), generator=g, dtype=torch.int32)
    idx[torch.rand(idx.shape, generator=g) < 1 / 9] = -1
    idx = idx.to(DEV)
    cu, lens, kw = lens_of(CU), lens_of(LENS), dict(scale=SCALE, num_splits=n, variant=variant)
    packed = fa.flash_attention_mla_sparse_varlen_decode_forward
    O, L = packed(Q, KV8, idx, cu, MAX_Q, lens, DEV, kv_format="fp8_ds", **kw)
    O16, L16 = packed(Q, fa.dequantize_mla_cache_ds(KV8, dtype), idx, cu, MAX_Q, lens, DEV, **kw)
    own = CU[-1]  # the rows some sequence owns: the others are not written
    assert not torch.isnan(O[:own].float()).any() and same_bits(O[:own], O16[:own]) and same_bits(L[:, :own], L16[:, :own])
    assert (L[:, CU[2]:CU[3]].float() == float("inf")).all() and (O[CU[2]:CU[3]] == 0).all()  # N_k = 0: empty rows
    for b in range(B):
        r0, r1 = CU[b], CU[b + 1]
        if r0 == r1:
            continue
        Ob, Lb = fa.flash_attention_mla_sparse_decode_forward(Q[r0:r1].transpose(0, 1)[None], KV8[b:b + 1], idx[r0:r1].transpose(0, 1)[None],
                                                              lens[b:b + 1], DEV, kv_format="fp8_ds", **kw)
        assert same_bits(Ob[0].transpose(0, 1), O[r0:r1]) and same_bits(Lb[0], L[:, r0:r1]), b
