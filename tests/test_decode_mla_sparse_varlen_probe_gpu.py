"""Sparse MLA decode of packed queries (fa2_fwd_kvcache_mla_sparse_varlen) through the exact-arithmetic probe of
tests/mla_sparse_varlen_probe.py, by flash_attention_mla_sparse_varlen_decode_forward: O within one output ulp of the fp64 truth on the
gathered rows, exact zeros where no listed key writes -- the value code names every key that reached the output, and with it the
sequence and the KV head it came from --, L within one ulp, rows without a valid entry O = 0 and L = +inf.  One ragged batch of 33
packed rows over at most 2560 keys -- a leading empty sequence, two in a row, a trailing one, a B that takes the owner search four
steps deep --, a quarter, a partial, one and two head tiles, topk 1 / 63 / 64 / 65 / 200 / 2048, two KV heads with lists of their own,
every split count and what num_splits = 0 resolves to, both kernel forms, both 16-bit dtypes and float32 on the VALU form, both fp8
formats under both codings, block tables of page size 1, 16, 48 and 64 with decoys in the spare pages, the lists as (total_q, topk)
and as a strided view, and max_seqlen_q below the longest chunk.  tests/test_decode_mla_sparse_varlen_gpu.py holds the packed call to
the fixed call bit for bit, with the same row expressions on both sides and on random data; this file pins the owner search, the
[t, h_kv] list address, the packed partial rows, the combine's packed walk and the (H, total_q) layout of L to values.
tests/test_decode_mla_sparse_varlen_probe.py shows on the CPU that each error of that layout fails these bars in every (packed row, KV
head) it changes."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_fp8_probe as P8
import mla_sparse_probe as S
import mla_sparse_varlen_probe as V
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
TOTAL, B = V.TOTAL, V.B

ids = lambda x: str(x).replace("torch.", "")


def cache(h_kv):
    """the latent rows (B, H_kv, S_k, 576) in float64, decoys behind N_K[b]: built once (mla_sparse_varlen_probe.cache), never modified"""
    return V.cache(h_kv, DEV)


@functools.lru_cache(maxsize=None)
def case(H, h_kv, topk, uniform):
    """packed Q (total_q, H, 576) in float64, the lists (total_q, H_kv, topk) and the fp64 truth O (total_q, H, 512), L (H, total_q) of
    one configuration: computed once, shared by every variant, dtype and cache form, never modified (c = 1 for the 16-bit dtypes and
    float32 alike)"""
    Q, K, keep = V.operands(H // h_kv, h_kv, topk, uniform, device=DEV)
    O, L = V.to_call(*V.truth(Q, K, keep, F32), h_kv)
    return V.packed_queries(H // h_kv, h_kv, uniform, DEV), V.lists(h_kv, topk, DEV), O, L


def broken(O, L, O_ref, L_ref, dtype, split, rows=None):
    """the bars the call's O (total_q, H, 512), L (H, total_q) break over `rows` (all), and the (packed row, sequence) pairs that break one"""
    rows = list(range(TOTAL)) if rows is None else rows
    col = lambda x: x.t().unsqueeze(-1)
    v = D.violations(O[rows], col(L)[rows], O_ref[rows], col(L_ref)[rows], dtype, split)
    if not v:
        return None
    return v, "(row, sequence)", [(t, V.OWNER[t]) for t in rows if D.violations(O[t:t + 1], col(L)[t:t + 1], O_ref[t:t + 1], col(L_ref)[t:t + 1],
                                                                                dtype, split)]


def run(dtype, variant, cfgs, cache_of, lists_of=lambda idx: idx):
    """the probe, scored and uniform, over `cfgs` on the latent cache cache_of(h_kv) (any form; with it the keyword arguments of that
    form) -> [(case, probe, violations, rows)]"""
    bad = []
    cu = torch.tensor(V.CU, dtype=torch.int32, device=DEV)
    lens = torch.tensor(V.N_K, dtype=torch.int32, device=DEV)
    for H, h_kv, topk, n in cfgs:
        resolved = n or _lib.kvcache_mla_sparse_varlen_num_splits(TOTAL, H, h_kv, topk, 576, 512, convert_triton_dtype(dtype))
        KV, extra = cache_of(h_kv)
        for uniform in (False, True):
            Q, idx, O_ref, L_ref = case(H, h_kv, topk, uniform)
            O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q.to(dtype), KV, lists_of(idx), cu, V.MAX_Q, lens, DEV, scale=D.SCALE,
                                                                       num_splits=n, variant=variant, **extra)
            assert O.shape == (TOTAL, H, 512) and L.shape == (H, TOTAL) and O.dtype == dtype and L.dtype == dtype
            v = broken(O, L, O_ref, L_ref, dtype, resolved > 1)
            if v:
                bad.append(((H, h_kv, topk, n, resolved), "uniform" if uniform else "scored") + v)
    return bad


FWD = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic")]


@pytest.mark.parametrize("rotation,dtype,variant", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_ragged_sparse_probe(rotation, dtype, variant):
    """every configuration, scored and uniform; each form and dtype under a rotation of its own, so that every configuration meets
    every split count, 0 and 1 among them"""
    cfgs = V.cases(rotation)
    assert [c[:3] for c in cfgs] == V.CONFIGS and len(FWD) >= len(V.SPLITS)
    bad = run(dtype, variant, cfgs, lambda h_kv: (cache(h_kv).to(dtype), {}))
    assert not bad, bad[:10]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=ids)
def test_every_split_count_meets_the_matrix_form(dtype):
    """topk 2048 over two head tiles and two KV heads of 128 heads each meet every split count on mla16"""
    assert V.CONFIGS[5] == (128, 1, 2048) and V.CONFIGS[7] == (256, 2, 200)
    cfgs = [cfg + (n,) for cfg in (V.CONFIGS[5], V.CONFIGS[7]) for n in V.SPLITS]
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
def test_ragged_sparse_probe_fp8_cache(rotation, fmt, descale, variant):
    """the same rows stored as KV / 2 under kv_descale 2 or as 4 KV under 0.25, exact in e4m3fn and e5m2: the same truth and bars"""
    dtype = (BF16, F16)[(rotation // 2) % 2]
    bad = run(dtype, variant, V.cases(rotation), lambda h_kv: (stored(h_kv, descale, fmt), dict(kv_descale=descales(h_kv, descale))))
    assert not bad, bad[:10]


PAGED = [(p, v, dt, f8) for p, dt, f8 in ((1, BF16, None), (16, F16, None), (48, BF16, E4), (64, F16, None)) for v in ("mla16", "generic")]


@pytest.mark.parametrize("rotation,page,variant,dtype,fmt", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_ragged_sparse_probe_paged(rotation, page, variant, dtype, fmt):
    """the latent cache behind a shuffled block table of any page size; the spare pages and the tail of a last page hold decoys (rows of
    the sequence without a key).  Page size 48 runs over an fp8 pool, scattered as bytes."""
    def cache_of(h_kv):
        if fmt is None:
            pool, table = S.pool(cache(h_kv).to(dtype), page, 7 * page + h_kv, decoy=V.NO_KEYS_B)
            return pool, dict(block_table=table)
        pool, table = S.pool(stored(h_kv, 0.25, fmt).view(torch.uint8), page, 7 * page + h_kv, decoy=V.NO_KEYS_B)
        return pool.view(fmt), dict(block_table=table, kv_descale=descales(h_kv, 0.25))
    bad = run(dtype, variant, V.cases(rotation), cache_of)
    assert not bad, bad[:10]


@pytest.mark.parametrize("variant", ["mla16", "generic"])
def test_lists_as_the_indexer_returns_them_and_as_a_strided_view(variant):
    """(total_q, topk) for one KV head -- the indexer's shape --, and (total_q, H_kv, topk) as a view of every other element of a wider
    tensor (no unit stride, rows and heads apart by more than topk): the same truth and bars"""
    H, h_kv, topk = V.CONFIGS[3]
    assert h_kv == 1
    bad = run(BF16, variant, [(H, h_kv, topk, 3)], lambda h: (cache(h).to(BF16), {}), lambda idx: idx[:, 0])
    assert not bad, bad

    def strided(idx):
        wide = torch.full((TOTAL, idx.shape[1], 2 * idx.shape[2] + 3), 7, dtype=torch.int32, device=DEV)   # (7: a key of most sequences)
        wide[:, :, 1:2 * idx.shape[2] + 1:2] = idx
        view = wide[:, :, 1:2 * idx.shape[2] + 1:2]
        assert not view.is_contiguous() and torch.equal(view, idx)
        return view
    bad = run(F16, variant, [V.CONFIGS[4] + (3,), V.CONFIGS[7] + (1,)], lambda h: (cache(h).to(F16), {}), strided)
    assert not bad, bad


@pytest.mark.parametrize("variant,dtype,k,max_q", [("mla16", BF16, 5, 3), ("mla16", F16, 4, 4), ("generic", BF16, 1, 3)], ids=ids)
def test_max_seqlen_q_below_the_longest_chunk(variant, dtype, k, max_q):
    """sequence b owns min(n_q(b), max_seqlen_q) rows from cu_seqlens_q[b] on: they meet the bars of the truth (a list's arithmetic does
    not depend on the chunk length), every other row of O and L keeps a sentinel, in the one-split path and across one multi-split
    call; rows of a packed tensor longer than cu_seqlens_q[B] belong to no sequence and keep it too.  Through the entry point itself,
    on outputs the test fills."""
    H, h_kv, topk = V.CONFIGS[k]
    assert max_q < V.MAX_Q
    tail = 2                                                                             # rows behind the last offset
    owned = [t for t in range(TOTAL) if V.POS[t] < max_q]
    rest = [t for t in range(TOTAL + tail) if t not in owned]
    assert len(owned) < TOTAL and any(V.N_Q[b] > max_q for b in range(B))
    cu = torch.tensor(V.CU, dtype=torch.int32, device=DEV)
    lens = torch.tensor(V.N_K, dtype=torch.int32, device=DEV)
    KV = cache(h_kv).to(dtype)
    enum = convert_triton_dtype(dtype)
    for n in (1, 3):
        for uniform in (False, True):
            Q, idx, O_ref, L_ref = case(H, h_kv, topk, uniform)
            Qd = torch.ones(TOTAL + tail, H, 576, dtype=dtype, device=DEV)               # rows of no sequence: not read
            Qd[owned] = Q.to(dtype)[owned]
            ix = torch.zeros(TOTAL + tail, h_kv, topk, dtype=torch.int32, device=DEV)
            ix[:TOTAL] = idx
            O = torch.full((TOTAL + tail, H, 512), 77.0, dtype=dtype, device=DEV)
            L = torch.full((H, TOTAL + tail), 77.0, dtype=dtype, device=DEV)
            ws = torch.empty(max(_lib.kvcache_varlen_workspace_bytes(TOTAL + tail, H, 512, n) // 4, 16), dtype=F32, device=DEV)
            _lib.fa2_fwd_kvcache_mla_sparse_varlen(Qd, KV, KV[..., :512], O, L, ix, cu, max_q, lens, enum, enum, scale=D.SCALE, num_splits=n,
                                                   workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
            torch.cuda.synchronize()
            assert (O[rest] == 77.0).all() and (L[:, rest] == 77.0).all(), (n, uniform)
            v = broken(O[:TOTAL], L[:, :TOTAL], O_ref, L_ref, dtype, n > 1, owned)
            assert not v, (n, "uniform" if uniform else "scored", v)
