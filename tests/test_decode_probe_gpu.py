"""Every KV-cache decode form through the exact-arithmetic probe (oracle/fa2_decode_probe.py): O within one output ulp of the
fp64 truth, exact zeros where no visible key writes, L within one ulp, empty rows O = 0 and L = +inf -- over the packed rows of a
KV group, splits and the combine launch, key groups inside a workgroup, decoy rows behind cache_seqlens, fp8 staging with
descales, the block table and strided layouts.  tests/test_decode_probe.py shows on the CPU that a wrong, missing or repeated key,
V tile, row, KV head, length or descale fails these bars on every case run here.  All calls go through
flash_attention_kvcache_forward, one batch of all lengths with two KV heads each."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
E4, E5 = D.F8
B = len(D.LENS)
SPARE = 5  # pool pages no table names: decoy rows

ids = lambda x: str(x).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def cache(d):
    """the probe's K, V (B, H_kv, S_k, d) in float64, decoys behind N_k(b): built once per head size, never modified"""
    return D.probe_cache(d, device=DEV)


@functools.lru_cache(maxsize=None)
def case(d, g, n_q, causal, window, uniform, c64):
    """Q (B, H, N_q, d) in float64 and the fp64 truth O (B, H, N_q, d), L (B, H, N_q, 1) of one configuration: computed once,
    shared by every variant, dtype and cache form, never modified (c64: with float64 I/O's c = 1 + 2.7e-9)"""
    K, V = cache(d)
    Q = D.probe_queries(g, n_q, d, uniform, device=DEV)
    keep = D.decode_keep(g, n_q, causal, window, device=DEV)
    O, L = D.truth(Q, K, V, keep, F64 if c64 else F32)
    return D.to_heads(Q, g, n_q), D.to_heads(O, g, n_q), D.to_heads(L, g, n_q)


def lens_of(values=D.LENS):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def covers_the_grid(cfgs):
    """every split count, and packed row counts on both sides of one 32-row block"""
    return {c[4] for c in cfgs} == set(D.SPLITS) and {c[0] * c[1] > 32 for c in cfgs} == {False, True}


def run(dtype, variant, d, cfgs, K, V, **kw):
    """the probe, scored and uniform, over `cfgs` on the cache K, V (any form) -> [(case, probe, violations)]"""
    bad = []
    lens = lens_of()
    for g, n_q, causal, window, n in cfgs:
        resolved = n or _lib.kvcache_num_splits(B, g * D.H_KV, D.H_KV, n_q, D.S_K, d, convert_triton_dtype(dtype))
        for uniform in (False, True):
            Q, O_ref, L_ref = case(d, g, n_q, causal, window, uniform, dtype == F64)
            O, L = fa.flash_attention_kvcache_forward(Q.to(dtype), K, V, lens, DEV, causal=causal, scale=D.SCALE, window=window,
                                                      num_splits=n, variant=variant, **kw)
            assert O.shape == Q.shape and O.dtype == dtype and L.dtype == dtype
            v = D.violations(O, L, O_ref, L_ref, dtype, resolved > 1)
            if v:
                bad.append(((g, n_q, causal, window, n, resolved), "uniform" if uniform else "scored", v))
    return bad


FWD = [(dt, v, d) for dt in (F16, BF16) for v in ("auto", "generic", "mfma16") for d in (64, 128)]
FWD += [(dt, "generic", d) for dt in (F32, F64) for d in (64, 40)]


@pytest.mark.parametrize("rotation,dtype,variant,d", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_decode_probe(rotation, dtype, variant, d):
    cfgs = D.cases(rotation, valu=variant == "generic")        # (the 80-row and the three-tile case: the VALU form only)
    assert covers_the_grid(cfgs)
    K, V = (t.to(dtype) for t in cache(d))
    bad = run(dtype, variant, d, cfgs, K, V)
    assert not bad, bad[:10]


def descales(shape=(B, D.H_KV)):
    return {"k_descale": torch.full(shape, D.K_DESCALE, device=DEV), "v_descale": torch.full(shape, D.V_DESCALE, device=DEV)}


FP8 = [(fmt, dt, v, d) for fmt in (E4, E5) for dt in (BF16, F16) for v in ("mfma16", "generic") for d in (64, 128)]


@pytest.mark.parametrize("rotation,fmt,dtype,variant,d", [(k,) + c for k, c in enumerate(FP8)], ids=ids)
def test_decode_probe_fp8_cache(rotation, fmt, dtype, variant, d):
    """K8 = K / 2 under k_descale 2, V8 = 4 V under v_descale 0.25: the same truth, and a descale dropped or swapped shows"""
    cfgs = D.cases(rotation)
    assert covers_the_grid(cfgs)
    K8, V8 = D.fp8_cache(*cache(d), fmt)
    bad = run(dtype, variant, d, cfgs, K8, V8, **descales())
    if rotation % 4 == 0:  # (B, 1)-shaped descales
        bad += run(dtype, variant, d, cfgs[:2], K8, V8, **descales((B, 1)))
    assert not bad, bad[:10]


def scatter(K, V, page, seed):
    """the contiguous cache scattered into pools of B * max_blocks + SPARE pages under a seeded random permutation table ->
    (K_pool, V_pool, table).  The rows behind N_k(b) keep the cache's decoys; the spare pages hold decoy rows as well (the pages
    of sequence 0, whose length is 0)."""
    Bc, h_kv, s_k, d = K.shape
    mb = s_k // page
    assert mb * page == s_k and D.LENS[0] == 0
    nb = Bc * mb + SPARE
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:Bc * mb].view(Bc, mb)
    pools = []
    for t in (K, V):
        raw = t.view(torch.uint8) if t.dtype in D.F8 else t
        pages = raw.view(Bc, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(Bc * mb, h_kv, page, d)
        pool = torch.empty(nb, h_kv, page, d, dtype=raw.dtype, device=DEV)
        pool[table.view(-1)] = pages
        pool[perm[Bc * mb:]] = pages[:SPARE]
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], table.to(torch.int32).contiguous()


PAGED = [(64, "mfma16", BF16, None, 128), (128, "mfma16", F16, None, 64), (16, "generic", BF16, None, 64),
         (64, "mfma16", F16, E4, 64), (128, "mfma16", BF16, E4, 128), (16, "generic", F16, E4, 128)]
PAGED_CONFIGS = (0, 2, 5, 6)  # no mask at R 4 and 64, a causal window at R 40, a two-sided window under causal at R 16


@pytest.mark.parametrize("rotation,page,variant,dtype,fmt,d", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_decode_probe_paged(rotation, page, variant, dtype, fmt, d):
    """the probe's cache behind a shuffled block table: the probe bars, not bit-identity with the contiguous call"""
    cfgs = [c for k, c in enumerate(D.cases(rotation)) if k in PAGED_CONFIGS]
    K, V = D.fp8_cache(*cache(d), fmt) if fmt else (t.to(dtype) for t in cache(d))
    Kp, Vp, table = scatter(K, V, page, 7 * page + d)
    bad = run(dtype, variant, d, cfgs, Kp, Vp, block_table=table, **(descales() if fmt else {}))
    assert not bad, bad[:10]


def test_decode_probe_bshd_cache_and_bnhd_query():
    """a (B, S, H_kv, d) cache and a (B, N_q, H, d) query viewed head-first, bf16, auto"""
    d = 128
    bshd = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    K, V = (bshd(t.to(BF16)) for t in cache(d))
    assert K.stride(2) == D.H_KV * d and not K.is_contiguous()
    bad = []
    lens = lens_of()
    for g, n_q, causal, window, n in D.cases(3):
        for uniform in (False, True):
            Q, O_ref, L_ref = case(d, g, n_q, causal, window, uniform, False)
            Qv = bshd(Q.to(BF16))
            assert Qv.stride(1) == d
            O, L = fa.flash_attention_kvcache_forward(Qv, K, V, lens, DEV, causal=causal, scale=D.SCALE, window=window, num_splits=n)
            resolved = n or _lib.kvcache_num_splits(B, g * D.H_KV, D.H_KV, n_q, D.S_K, d, convert_triton_dtype(BF16))
            v = D.violations(O, L, O_ref, L_ref, BF16, resolved > 1)
            if v:
                bad.append(((g, n_q, causal, window, n), "uniform" if uniform else "scored", v))
    assert not bad, bad[:10]
