"""Packed (ragged) queries over the latent cache (fa2_fwd_kvcache_mla_varlen) through the exact-arithmetic probe of
tests/mla_varlen_probe.py, by flash_attention_mla_varlen_decode_forward, on the ragged batch and the configurations of
tests/test_decode_mla_varlen_gpu.py: O within one output ulp of the fp64 truth, exact zeros where no visible key writes, L within
one ulp, empty rows O = 0 and L = +inf -- for both kernel forms, both 16-bit dtypes, float32 on the VALU form, every split count
and what num_splits = 0 resolves to, both fp8 formats under both codings, page sizes 16 / 64 / 256, and max_seqlen_q below the
longest chunk.  Random data at these lengths cannot see a dropped 64-key tile, a band one key off, a wrong split edge or a row that
answers with its neighbour's keys, and that file's bit-identities run the same row map on both sides; this file pins the
position-major row map, the tiles that cut a position, the per-tile key clip, the shift from n_q(b), the partial row, the x
rotation and the combine's packed walk to values.  tests/test_decode_mla_varlen_probe.py shows on the CPU that each error of that
layout fails these bars in every sequence it changes.  One batch of 163 rows over at most 2560 keys."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_fp8_probe as P8
import mla_probe as M
import mla_varlen_probe as V
import test_decode_mla_varlen_gpu as G
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
B, TOTAL, CU = V.B, V.TOTAL, V.CU
SPARE = 5  # pool pages no table names: decoy rows

ids = lambda x: str(x).replace("torch.", "")


def test_the_batch_is_the_helper_s():
    assert (G.N_Q, G.N_K, G.S_K, G.MAX_Q, G.TOTAL) == (V.N_Q, V.N_K, V.S_K, V.MAX_Q, V.TOTAL)
    assert G.CONFIGS == V.CONFIGS and G.SPLITS == V.SPLITS and G.WINDOWS == V.WINDOWS


def cache(h_kv):
    """the latent rows (B, H_kv, S_k, 576) in float64, decoys behind N_K[b]: built once (mla_varlen_probe.cache), never modified"""
    return V.cache(h_kv, DEV)


@functools.lru_cache(maxsize=None)
def case(g, h_kv, causal, window, uniform, n_q=tuple(V.N_Q)):
    """packed Q (total_q, H, 576) in float64 and the fp64 truth O (total_q, H, 512), L (total_q, H, 1) of one configuration, every
    sequence with its own n_q(b) (n_q: other chunk lengths than the batch's, packed at the batch's offsets, the rows between them
    zero): computed once, shared by every variant, dtype and cache form, never modified (c = 1 for the 16-bit dtypes and float32
    alike)"""
    Q = torch.zeros(TOTAL, g * h_kv, M.D_QK, dtype=torch.float64, device=DEV)
    O = torch.zeros(TOTAL, g * h_kv, M.D_V, dtype=torch.float64, device=DEV)
    L = torch.zeros(TOTAL, g * h_kv, 1, dtype=torch.float64, device=DEV)
    for b, nq in enumerate(n_q):
        if nq:
            Qb, KV = V.seq_queries(g, nq, uniform, h_kv, DEV), V.seq_cache(h_kv, b, DEV)
            keep = M.decode_keep(g, nq, causal, window, lens=[V.N_K[b]] * h_kv, s_k=V.S_K, device=DEV)
            Ob, Lb = M.mla_truth(Qb, KV, keep, F32)
            for dst, src in ((Q, Qb), (O, Ob), (L, Lb)):
                dst[CU[b]:CU[b] + nq] = V.pack(src, g, nq)
    return Q, O, L


def broken(O, L, O_ref, L_ref, dtype, split, n_q=V.N_Q):
    """the bars the call's O (total_q, H, 512), L (H, total_q) break, and the sequences that break one"""
    Lt = L.t().unsqueeze(-1).contiguous()
    rows = torch.cat([torch.arange(CU[b], CU[b] + nq) for b, nq in enumerate(n_q)]).to(DEV)
    v = M.violations(O[rows], Lt[rows], O_ref[rows], L_ref[rows], dtype, split)
    if not v:
        return None
    return v, "sequences", [b for b, nq in enumerate(n_q) if nq and M.violations(O[CU[b]:CU[b] + nq], Lt[CU[b]:CU[b] + nq], O_ref[CU[b]:CU[b] + nq],
                                                                                L_ref[CU[b]:CU[b] + nq], dtype, split)]


def run(dtype, variant, cfgs, cache_of, **kw):
    """the probe, scored and uniform, over `cfgs` on the latent cache cache_of(h_kv) (any form; with it the keyword arguments of
    that form) -> [(case, probe, violations, sequences)]"""
    bad = []
    cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
    lens = torch.tensor(V.N_K, dtype=torch.int32, device=DEV)
    for g, h_kv, causal, window, n in cfgs:
        H = g * h_kv
        resolved = n or _lib.kvcache_mla_varlen_num_splits(B, H, h_kv, TOTAL, V.MAX_Q, V.S_K, 576, 512, convert_triton_dtype(dtype))
        KV, extra = cache_of(h_kv)
        for uniform in (False, True):
            Q, O_ref, L_ref = case(g, h_kv, causal, window, uniform)
            O, L = fa.flash_attention_mla_varlen_decode_forward(Q.to(dtype), KV, cu, V.MAX_Q, lens, DEV, causal=causal, scale=D.SCALE,
                                                                window=window, num_splits=n, variant=variant, **extra, **kw)
            assert O.shape == (TOTAL, H, 512) and L.shape == (H, TOTAL) and O.dtype == dtype and L.dtype == dtype
            v = broken(O, L, O_ref, L_ref, dtype, resolved > 1)
            if v:
                bad.append(((g, h_kv, causal, window, n, resolved), "uniform" if uniform else "scored") + v)
    return bad


FWD = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic")]


@pytest.mark.parametrize("rotation,dtype,variant", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_ragged_mla_probe(rotation, dtype, variant):
    """every configuration, scored and uniform; over the seven cases each configuration meets every split count, 0 and 1 among them"""
    cfgs = V.cases(rotation)
    assert [c[:4] for c in cfgs] == V.CONFIGS and {c[4] for c in cfgs} == set(V.SPLITS) and len(FWD) == len(V.SPLITS)
    bad = run(dtype, variant, cfgs, lambda h_kv: (cache(h_kv).to(dtype), {}))
    assert not bad, bad[:10]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=ids)
def test_every_split_count_meets_the_matrix_form(dtype):
    """over the rotations of test_ragged_mla_probe a configuration meets each split count on one form and dtype; here a causal
    configuration whose 64-row tiles cut a position (g 40: 1.6 positions a tile, up to 44 row tiles a sequence) meets all on mla16"""
    cfgs = [(40, 1, True, None, n) for n in V.SPLITS]
    bad = run(dtype, "mla16", cfgs, lambda h_kv: (cache(h_kv).to(dtype), {}))
    assert not bad, bad[:10]


@functools.lru_cache(maxsize=None)
def stored(h_kv, descale, fmt):
    """the latent rows in fp8 under kv_descale = descale: built once, never modified"""
    KV8 = P8.stored(cache(h_kv), descale, fmt)
    assert torch.equal(P8.dequantised(KV8, descale), cache(h_kv))
    return KV8


def descales(h_kv, descale):
    return torch.full((B, h_kv), descale, dtype=torch.float32, device=DEV)


FP8 = [(fmt, descale, variant) for fmt in (E4, E5) for descale in P8.CODINGS for variant in ("mla16", "generic")]


@pytest.mark.parametrize("rotation,fmt,descale,variant", [(k,) + c for k, c in enumerate(FP8)], ids=ids)
def test_ragged_mla_probe_fp8_cache(rotation, fmt, descale, variant):
    """the same rows stored as KV / 2 under kv_descale 2 or as 4 KV under 0.25, exact in e4m3fn and e5m2: the same truth and bars"""
    dtype = (BF16, F16)[(rotation // 2) % 2]
    bad = run(dtype, variant, V.cases(rotation), lambda h_kv: (stored(h_kv, descale, fmt), dict(kv_descale=descales(h_kv, descale))))
    assert not bad, bad[:10]


def scatter(KV, page, seed):
    """the contiguous latent cache scattered into a pool of B * max_blocks + SPARE pages under a seeded random permutation table ->
    (pool, table); the spare pages hold decoy rows (pages of the sequence whose length is 0), and so do the rows behind N_K[b]"""
    Bc, h_kv, s_k, d = KV.shape
    mb = s_k // page
    empty = V.N_K.index(0)
    assert mb * page == s_k and SPARE <= mb
    nb = Bc * mb + SPARE
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:Bc * mb].view(Bc, mb)
    pages = KV.view(Bc, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(Bc * mb, h_kv, page, d)
    pool = torch.empty(nb, h_kv, page, d, dtype=KV.dtype, device=DEV)
    pool[table.view(-1)] = pages
    pool[perm[Bc * mb:]] = pages[empty * mb:empty * mb + SPARE]
    return pool, table.to(torch.int32).contiguous()


PAGED = [(64, "mla16", BF16, None), (256, "mla16", F16, None), (16, "generic", BF16, None), (64, "mla16", F16, E4), (16, "generic", BF16, E5)]


@pytest.mark.parametrize("rotation,page,variant,dtype,fmt", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_ragged_mla_probe_paged(rotation, page, variant, dtype, fmt):
    """the latent cache behind a shuffled block table, decoy rows behind N_K[b] and in the spare pages (fp8: scattered as bytes)"""
    def cache_of(h_kv):
        if fmt is None:
            pool, table = scatter(cache(h_kv).to(dtype), page, 7 * page + h_kv)
            return pool, dict(block_table=table)
        pool, table = scatter(stored(h_kv, 0.25, fmt).view(torch.uint8), page, 7 * page + h_kv)
        return pool.view(fmt), dict(block_table=table, kv_descale=descales(h_kv, 0.25))
    bad = run(dtype, variant, V.cases(rotation + 2), cache_of)
    assert not bad, bad[:10]


@pytest.mark.parametrize("variant,dtype,g,h_kv,causal,window,max_q", [("mla16", BF16, 40, 1, True, None, 50), ("mla16", F16, 16, 2, True, (64, 0), 3),
                                                                      ("generic", BF16, 5, 1, False, (64, 0), 50)], ids=ids)
def test_max_seqlen_q_below_the_longest_chunk(variant, dtype, g, h_kv, causal, window, max_q):
    """sequence b owns min(n_q(b), max_seqlen_q) rows from cu_seqlens_q[b] on: they meet the bars of the truth at THAT chunk length
    (the bottom-right shift, the row map and the row tiles are those of the clipped chunk), every other row of O and L keeps a
    sentinel.  Through the entry point itself, on outputs the test fills."""
    own = tuple(min(nq, max_q) for nq in V.N_Q)
    assert own != tuple(V.N_Q) and max(own) == max_q
    H = g * h_kv
    cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
    lens = torch.tensor(V.N_K, dtype=torch.int32, device=DEV)
    live = torch.zeros(TOTAL, dtype=torch.bool, device=DEV)
    for b, nq in enumerate(own):
        live[CU[b]:CU[b] + nq] = True
    KV = cache(h_kv).to(dtype)
    enum = convert_triton_dtype(dtype)
    for n in (1, 3):
        for uniform in (False, True):
            Q, O_ref, L_ref = case(g, h_kv, causal, window, uniform, own)
            Qd = Q.to(dtype)
            Qd[~live] = 1.0                                                             # rows of no sequence: not read
            O = torch.full((TOTAL, H, 512), 77.0, dtype=dtype, device=DEV)
            L = torch.full((H, TOTAL), 77.0, dtype=dtype, device=DEV)
            ws = torch.empty(max(_lib.kvcache_varlen_workspace_bytes(TOTAL, H, 512, n) // 4, 16), dtype=F32, device=DEV)
            _lib.fa2_fwd_kvcache_mla_varlen(Qd, KV, O, L, cu, max_q, lens, enum, enum, 512, causal=causal, scale=D.SCALE, window=window,
                                            num_splits=n, workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
            torch.cuda.synchronize()
            assert (O[~live] == 77.0).all() and (L[:, ~live] == 77.0).all(), (n, uniform)
            v = broken(O, L, O_ref, L_ref, dtype, n > 1, own)
            assert not v, (n, "uniform" if uniform else "scored", v)
