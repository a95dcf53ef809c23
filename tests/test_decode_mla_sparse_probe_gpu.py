"""Sparse MLA decode (fa2_fwd_kvcache_mla_sparse) through the exact-arithmetic probe of tests/mla_sparse_probe.py, by the Python
surface: O within one output ulp of the fp64 truth on the gathered rows, exact zeros where no listed key writes -- the value code
names every key that reached the output --, L within one ulp, rows without a valid entry O = 0 and L = +inf; over a quarter, a partial,
one and two head tiles, every topk of the grid, splits over the slots and the combine launch, entries that are no key, decoy rows
behind cache_seqlens, and block tables of page size 1, 16, 48 and 64 under both forms with decoys in the spare pages.
tests/test_decode_mla_sparse_probe.py shows on the CPU that every planted gather error fails these bars on every case run here."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_sparse_probe as S
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32

ids = lambda x: str(x).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def cache():
    """the latent rows (B, 1, S_K, 576) in float64, decoys behind N_k(b): built once, never modified"""
    return S.latent_cache(device=DEV)


@functools.lru_cache(maxsize=None)
def case(H, n_q, topk, uniform):
    """Q (B, H, N_q, 576) in float64, the lists and the fp64 truth O (B, H, N_q, 512), L (B, H, N_q, 1): computed once, shared by
    every variant, dtype and cache form, never modified (c = 1 for the 16-bit dtypes and float32 alike)"""
    idx = S.lists(n_q, topk, device=DEV)
    K, keep = S.gather(cache()[:, 0], idx, S.valid(idx), H)
    Q = S.gathered_queries(H, n_q, uniform, device=DEV)
    O, L = S.truth(Q, K, keep, F32)
    return S.to_call(Q, n_q).contiguous(), idx, S.to_call(O, n_q), S.to_call(L, n_q)


def run(dtype, variant, cfgs, KV, **kw):
    """the probe, scored and uniform, over `cfgs` on the latent cache KV (any form) -> [(case, probe, violations)]"""
    bad = []
    lens = torch.tensor(list(S.LENS), dtype=torch.int32, device=DEV)
    for H, n_q, topk, n in cfgs:
        resolved = n or _lib.kvcache_mla_sparse_num_splits(S.B, H, 1, n_q, topk, 576, 512, convert_triton_dtype(dtype))
        for uniform in (False, True):
            Q, idx, O_ref, L_ref = case(H, n_q, topk, uniform)
            O, L = fa.flash_attention_mla_sparse_decode_forward(Q.to(dtype), KV, idx, lens, DEV, scale=D.SCALE, num_splits=n,
                                                                variant=variant, **kw)
            assert O.shape == (S.B, H, n_q, 512) and O.dtype == dtype and L.dtype == dtype
            v = D.violations(O, L, O_ref, L_ref, dtype, resolved > 1)
            if v:
                bad.append(((H, n_q, topk, n, resolved), "uniform" if uniform else "scored", v))
    return bad


FWD = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic")]


@pytest.mark.parametrize("rotation,dtype,variant", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_sparse_probe(rotation, dtype, variant):
    cfgs = S.cases(rotation)
    assert [c[:3] for c in cfgs] == S.CONFIGS
    bad = run(dtype, variant, cfgs, cache().to(dtype))
    assert not bad, bad[:10]


def test_every_split_count_meets_the_matrix_form():
    """over the rotations of test_sparse_probe each configuration meets some split counts; here two with two head tiles meet all"""
    cfgs = [cfg + (n,) for cfg in (S.CONFIGS[5], S.CONFIGS[7]) for n in S.SPLITS]
    bad = run(BF16, "mla16", cfgs, cache().to(BF16))
    assert not bad, bad[:10]


PAGED = [(p, v, dt) for p, dt in ((1, BF16), (16, F16), (48, BF16), (64, F16)) for v in ("mla16", "generic")]


@pytest.mark.parametrize("rotation,page,variant,dtype", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_sparse_probe_paged(rotation, page, variant, dtype):
    """the latent cache behind a shuffled block table of any page size, spare pages holding decoys: the probe bars, every configuration"""
    pool, table = S.pool(cache().to(dtype), page, 7 * page)
    bad = run(dtype, variant, S.cases(rotation), pool, block_table=table)
    assert not bad, bad[:10]
