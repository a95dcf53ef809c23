"""MLA decode (fa2_fwd_kvcache_mla) through the exact-arithmetic probe of tests/mla_probe.py, by the Python surface: O within one
output ulp of the fp64 truth, exact zeros where no visible key writes, L within one ulp, empty rows O = 0 and L = +inf -- over one,
two and four 64-row tiles and a last partial one, splits and the combine launch, decoy rows behind cache_seqlens, the value
operand read from the key's own rows, and the block table.  tests/test_decode_mla_probe.py shows on the CPU that a score column
or k-step left out, a shifted V, exchanged value blocks, row tiles or rows, a stale row, a dropped tile and top-left alignment
fail these bars on every case run here.  One batch of the probe's 21 lengths at capacity 2560, H_kv = 1."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_probe as M
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
B = len(M.LENS)
SPARE = 5  # pool pages no table names: decoy rows

ids = lambda x: str(x).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def cache():
    """the latent rows (B, 1, S_k, 576) in float64, decoys behind N_k(b): built once, never modified"""
    return M.latent_cache(device=DEV)


@functools.lru_cache(maxsize=None)
def case(H, n_q, causal, window, uniform):
    """Q (B, H, N_q, 576) in float64 and the fp64 truth O (B, H, N_q, 512), L (B, H, N_q, 1): computed once, shared by every
    variant, dtype and cache form, never modified (c = 1 for the 16-bit dtypes and float32 alike)"""
    Q = M.queries(H, n_q, uniform, device=DEV)
    keep = M.decode_keep(H, n_q, causal, window, device=DEV)
    O, L = M.mla_truth(Q, cache(), keep, F32)
    return D.to_heads(Q, H, n_q), D.to_heads(O, H, n_q), D.to_heads(L, H, n_q)


def run(dtype, variant, cfgs, KV, **kw):
    """the probe, scored and uniform, over `cfgs` on the latent cache KV (any form) -> [(case, probe, violations)]"""
    bad = []
    lens = torch.tensor(list(M.LENS), dtype=torch.int32, device=DEV)
    for H, n_q, causal, window, n in cfgs:
        resolved = n or _lib.kvcache_mla_num_splits(B, H, 1, n_q, M.S_K, 576, 512, convert_triton_dtype(dtype))
        for uniform in (False, True):
            Q, O_ref, L_ref = case(H, n_q, causal, window, uniform)
            O, L = fa.flash_attention_mla_decode_forward(Q.to(dtype), KV, lens, DEV, causal=causal, scale=D.SCALE, window=window,
                                                         num_splits=n, variant=variant, **kw)
            assert O.shape == (B, H, n_q, 512) and O.dtype == dtype and L.dtype == dtype
            v = M.violations(O, L, O_ref, L_ref, dtype, resolved > 1)
            if v:
                bad.append(((H, n_q, causal, window, n, resolved), "uniform" if uniform else "scored", v))
    return bad


FWD = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic")]


@pytest.mark.parametrize("rotation,dtype,variant", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_mla_probe(rotation, dtype, variant):
    cfgs = M.cases(rotation)
    assert [c[:4] for c in cfgs] == M.CONFIGS and len({c[4] for c in cfgs}) == len(cfgs)
    bad = run(dtype, variant, cfgs, cache().to(dtype))
    assert not bad, bad[:10]


def test_every_split_count_meets_the_matrix_form():
    """over the rotations of test_mla_probe each configuration meets some split counts; here the two-tile causal case meets all"""
    cfgs = [M.CONFIGS[3] + (n,) for n in M.SPLITS]
    bad = run(BF16, "mla16", cfgs, cache().to(BF16))
    assert not bad, bad[:10]


def scatter(KV, page, seed):
    """the contiguous latent cache scattered into a pool of B * max_blocks + SPARE pages under a seeded random permutation table ->
    (pool, table); the spare pages hold decoy rows (the pages of sequence 0, whose length is 0)"""
    Bc, h_kv, s_k, d = KV.shape
    mb = s_k // page
    assert mb * page == s_k and M.LENS[0] == 0
    nb = Bc * mb + SPARE
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:Bc * mb].view(Bc, mb)
    pages = KV.view(Bc, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(Bc * mb, h_kv, page, d)
    pool = torch.empty(nb, h_kv, page, d, dtype=KV.dtype, device=DEV)
    pool[table.view(-1)] = pages
    pool[perm[Bc * mb:]] = pages[:SPARE]
    return pool, table.to(torch.int32).contiguous()


PAGED = [(64, "mla16", BF16), (128, "mla16", F16), (16, "generic", BF16)]


@pytest.mark.parametrize("rotation,page,variant,dtype", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_mla_probe_paged(rotation, page, variant, dtype):
    """the latent cache behind a shuffled block table: the probe bars, every configuration"""
    pool, table = scatter(cache().to(dtype), page, 7 * page)
    bad = run(dtype, variant, M.cases(rotation + 3), pool, block_table=table)
    assert not bad, bad[:10]
