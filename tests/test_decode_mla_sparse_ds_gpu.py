"""Sparse MLA decode over the tile-scaled fp8 cache (kv_format="fp8_ds") on the GPU.  The result is DEFINED as the 16-bit sparse call's
on dequantize_mla_cache_ds(KV8, T), bit for bit at the same variant and num_splits: no tolerance."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import check_forward, lens_of
from test_decode_mla_sparse_gpu import SCALE, lists, paged, same_bits, sparse_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16 = torch.float16, torch.bfloat16
S_K, LENS = 320, [0, 1, 63, 64, 65, 320]
# (H, H_kv, N_q, topk, num_splits, kind): "pow2" replaces the scales by powers of two, "dup" draws the lists from 40 positions, "heads"
# gives each KV head lists of its own; one slot in nine of every list is -1
CONFIGS = [(16, 1, 1, 1, 1, "rand"), (40, 1, 2, 63, 1, "pow2"), (64, 1, 1, 64, 3, "dup"), (128, 1, 2, 65, 3, "rand"), (32, 2, 2, 200, 0, "heads")]
ids = lambda x: str(x).replace("torch.", "")
sparse = fa.flash_attention_mla_sparse_decode_forward


def make_ds(B, H, H_kv, N_q, S_k, dtype, seed, pow2=False):
    """Q and an fp8_ds cache whose scales tell tiles and rows apart: column tile t of row j is drawn at magnitude 2^((j % 5) - 2 t), so
    the scales differ by factors of 4 between tiles and of 2 between rows, none a power of two.  All times 2^-4: check_forward's bars
    are absolute (6e-3 on f16) and at a top magnitude of 16 |O| reaches 18, where the 16-bit call itself misses them (1.9e-2)."""
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randn(B, H, N_q, 576, generator=g) * 0.5).to(dtype).to(DEV)
    mag = torch.exp2((torch.arange(S_k) % 5)[:, None].float() - 2 * torch.arange(4)[None].float() - 4).repeat_interleave(128, 1)
    x = torch.randn(B, H_kv, S_k, 576, generator=g) * torch.cat((mag, torch.full((S_k, 64), 0.5)), 1)
    KV8 = fa.quantize_mla_cache_ds(x.to(dtype).to(DEV))
    if pow2:
        s = KV8[..., 512:528].contiguous().view(torch.float32)
        KV8[..., 512:528] = torch.exp2(torch.log2(s).round()).view(torch.uint8)
    return Q, KV8


@functools.lru_cache(maxsize=None)
def case(dtype, cfg):
    H, H_kv, N_q, topk, _, kind = cfg
    Q, KV8 = make_ds(len(LENS), H, H_kv, N_q, S_K, dtype, 3 * H + topk, pow2=kind == "pow2")
    D = fa.dequantize_mla_cache_ds(KV8, dtype)
    idx = lists(len(LENS), H_kv, N_q, topk, kind, H + topk, s_k=S_K)
    return Q, KV8, D, idx, sparse_reference(Q, D.double(), D[..., :512].double(), idx, LENS, SCALE)


@pytest.mark.parametrize("cfg", CONFIGS, ids=ids)
@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_equals_the_16_bit_call_on_the_dequantised_cache_bit_for_bit(dtype, variant, cfg):
    Q, KV8, D, idx, (O_ref, L_ref) = case(dtype, cfg)
    s = KV8[..., 512:528].contiguous().view(torch.float32)
    assert (torch.log2(s) == torch.log2(s).round()).all() == (cfg[5] == "pow2") and (cfg[5] != "heads" or not torch.equal(idx[:, 0], idx[:, 1]))
    kw = dict(scale=SCALE, num_splits=cfg[4], variant=variant)
    O, L = sparse(Q, KV8, idx, lens_of(LENS), DEV, kv_format="fp8_ds", **kw)
    O16, L16 = sparse(Q, D, idx, lens_of(LENS), DEV, **kw)
    print(f"{ids(dtype)} {variant} {cfg}: {int((O.view(torch.int16) != O16.view(torch.int16)).sum())} of {O.numel()} elements of O differ")
    assert not torch.isnan(O.float()).any() and same_bits(O, O16) and same_bits(L, L16)
    if variant == "mla16":  # ... and against the fp64 truth on the dequantised rows: both calls wrong together
        check_forward(O, L, O_ref, L_ref, dtype, (dtype, cfg))


@pytest.mark.parametrize("page", [1, 16, 64])
@pytest.mark.parametrize("variant", ["mla16", "generic"])
def test_paged_equals_contiguous_bit_for_bit(variant, page):
    Q, KV8, _, idx, _ = case(BF16, CONFIGS[4])
    pool, table = paged(KV8, page, 33, fill=255.0)
    assert int((pool == 255).all(-1).all(-1).all(-1).sum()) >= 3
    for n in (1, 3):
        kw = dict(scale=SCALE, num_splits=n, variant=variant, kv_format="fp8_ds")
        O, L = sparse(Q, KV8, idx, lens_of(LENS), DEV, **kw)
        Op, Lp = sparse(Q, pool, idx, lens_of(LENS), DEV, block_table=table, **kw)
        assert not torch.isnan(Op.float()).any() and same_bits(O, Op) and same_bits(L, Lp), (variant, page, n)


@pytest.mark.parametrize("variant", ["mla16", "generic"])
def test_only_listed_rows_are_read(variant):
    """every byte and scale of every row no list names or behind N_k(b) set to 0x7f (NaN bytes), 0xff (NaN scales too) and +inf scales,
    under a poisoned workspace: not a bit of O or L moves"""
    Q, KV8, _, idx, _ = case(BF16, CONFIGS[3])
    H, N_q = Q.shape[1:3]
    named = torch.zeros(len(LENS), S_K, dtype=torch.bool, device=DEV)
    for b, nk in enumerate(LENS):
        j = idx[b].flatten().long()
        named[b, j[(j >= 0) & (j < nk)]] = True
    inf_row = torch.full((656,), 0x7f, dtype=torch.uint8, device=DEV)
    inf_row[512:528] = torch.full((4,), math.inf, device=DEV).view(torch.uint8)
    for n in (1, 3):
        results = []
        for poison in (None, 0x7f, 0xff, inf_row):
            cache = KV8.clone()
            if poison is not None:
                cache[:, 0][~named] = poison
            O, L = torch.empty(len(LENS), H, N_q, 512, dtype=BF16, device=DEV), torch.empty(len(LENS), H, N_q, dtype=BF16, device=DEV)
            ws = torch.full((max(_lib.kvcache_workspace_bytes(len(LENS), H, N_q, 512, n) // 4, 1),), math.nan, device=DEV)
            _lib.fa2_fwd_kvcache_mla_sparse_ds(Q, cache, O, L, idx, lens_of(LENS), convert_triton_dtype(BF16), scale=SCALE, num_splits=n, workspace=ws,
                                               variant=_lib.KVCACHE_MLA_VARIANTS[variant])
            results.append((O, L))
        assert not torch.isnan(results[0][0].float()).any()
        for O, L in results[1:]:
            assert same_bits(O, results[0][0]) and same_bits(L, results[0][1]), (variant, n)


def test_a_misaligned_view_runs_on_the_valu_form_and_the_forced_matrix_form_refuses_it():
    Q, KV8, _, idx, _ = case(BF16, CONFIGS[3])
    wide = torch.zeros(*KV8.shape[:3], 660, dtype=torch.uint8, device=DEV)
    view = wide[..., 4:]  # base + 4 bytes, a row stride of 660
    view.copy_(KV8)
    kw = dict(scale=SCALE, num_splits=3, kv_format="fp8_ds")
    with pytest.raises(TypeError, match="16 bytes"):  # FA2_ERR_UNSUPPORTED
        sparse(Q, view, idx, lens_of(LENS), DEV, variant="mla16", **kw)
    Og, Lg = sparse(Q, KV8, idx, lens_of(LENS), DEV, variant="generic", **kw)
    for variant in ("auto", "generic"):
        O, L = sparse(Q, view, idx, lens_of(LENS), DEV, variant=variant, **kw)
        assert same_bits(O, Og) and same_bits(L, Lg), variant
