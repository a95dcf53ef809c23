"""Packed (ragged) queries over the latent cache (fa2_fwd_kvcache_mla_varlen) on the GPU, one ragged batch of 0 to 70 query tokens
over 0 to 2560 keys: O and L against the fp64 per-sequence truth at the bars of tests/test_decode_gpu.py for both kernel forms,
every group size, mask and split count; bit-identities at equal explicit num_splits (every sequence alone against its rows in the
batch, the uniform batch against flash_attention_mla_decode_forward, paged against contiguous, fp8 at descale None against the
converted cache, the same call twice); stale rows, unused pages and a poisoned workspace that must not reach the output; canaries
around O, L and the workspace, packed rows outside every sequence untouched, inputs unchanged; fp8 caches with descales; the fused
ragged step against the append followed by the attention; strided and misaligned Q.  On the sequences of more than one key tile
or split, O is about 0.5 / sqrt(n) and these absolute bars cannot see a dropped 64-key tile, a band one key off, a wrong split edge
or a row answered with its neighbour's keys, and the bit-identities run the same row map on both sides:
tests/test_decode_mla_varlen_probe_gpu.py pins which keys each packed row reads, to one output ulp."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import arena, canaries_intact, f32, lens_of
from test_decode_gpu import check_forward as check_bhn
from test_decode_varlen_gpu import reference as reference_d

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2

D, D_V = 576, 512
S_K = 2560
N_Q = [0, 1, 3, 2, 5, 17, 1, 70, 64]
N_K = [100, 0, 2, 65, 64, 1000, S_K, 300, 64]
B, TOTAL, MAX_Q = len(N_Q), sum(N_Q), 70
SPLITS = (0, 1, 2, 3, 7, 16, 128)
WINDOWS = (None, (64, 0), (100, 50), (0, 0))
SCALE = D ** -0.5
# (g, H_kv, causal, window): a tile spanning many positions (g 1, 5, 16), a tile smaller than one position's heads (g 128), 64 % g != 0
# (g 5, 40), exactly one position per tile (g 64), two KV heads; every window, causal on and off; the split counts rotate over them
CONFIGS = [(1, 1, True, None), (5, 1, False, (64, 0)), (16, 1, True, (100, 50)), (40, 1, False, None), (64, 1, True, (0, 0)),
           (128, 1, False, (100, 50)), (16, 2, True, (64, 0)), (128, 1, True, None)]

ids = lambda x: str(x).replace("torch.", "")


def cu_of(n_q):
    return torch.tensor([0] + torch.tensor(list(n_q)).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def split_chunk(n_k, num_splits):
    return ((n_k + num_splits - 1) // num_splits + 63) & ~63


def test_the_batch_holds_every_class_of_length():
    pairs = list(zip(N_Q, N_K))
    assert max(N_Q) == MAX_Q and TOTAL == 163
    assert any(nq == 0 for nq in N_Q)                                                   # a sequence with no query
    assert any(nq > 0 and nk == 0 for nq, nk in pairs)                                  # N_k = 0
    assert any(0 < nk < nq for nq, nk in pairs)                                         # N_k < n_q: rows without a key under causal
    assert any(nq == nk == 64 for nq, nk in pairs)                                      # pure prefill of one whole key tile
    assert any(nk > nq > 0 and (nk - nq) // 64 != (nk - 1) // 64 for nq, nk in pairs)   # the chunk straddles a 64-key tile edge
    assert any(nk == S_K for nk in N_K)
    used = set(SPLITS[2:])
    for g, h_kv, _, _ in CONFIGS:  # what num_splits = 0 resolves to (the formula of tests/test_decode_mla_varlen_host.py)
        base = h_kv * min(B * -(-g * MAX_Q // 64), -(-g * TOTAL // 64) + B)
        used.add(1 if base >= 256 else max(1, min(-(-256 // base), S_K // 64 // 8, 128)))
    for n in sorted(used - {1}):                                                        # ... and a split edge, at every split count
        assert any(nk - nq < s * split_chunk(nk, n) < nk for nq, nk in pairs if nq > 1 for s in range(1, n)), n
    for g in {c[0] for c in CONFIGS}:                                                   # more than one row tile, a partly filled last one
        assert g * MAX_Q > 64 or g == 1
    assert {c[0] for c in CONFIGS} == {1, 5, 16, 40, 64, 128} and (16, 2) in {c[:2] for c in CONFIGS}
    assert {c[3] for c in CONFIGS} == set(WINDOWS) and {c[2] for c in CONFIGS} == {False, True}


@functools.lru_cache(maxsize=8)
def cache(h_kv, dtype, seed=1):
    g = torch.Generator().manual_seed(seed + h_kv)
    return (torch.randn(B, h_kv, S_K, D, generator=g) * 0.5).to(dtype).to(DEV)


@functools.lru_cache(maxsize=32)
def queries(g, h_kv, dtype, total=TOTAL):
    gen = torch.Generator().manual_seed(7 * g + h_kv)
    return (torch.randn(total, g * h_kv, D, generator=gen) * 0.5).to(dtype).to(DEV)


def reference(Q, KV, n_q, n_k, causal, scale, window, starts=None):
    """the fp64 truth of tests/test_decode_varlen_gpu.py widened for d_v: the value is the first D_V columns of the row, so the
    truth is the first D_V columns of P (KV)"""
    O, L = reference_d(Q, KV, KV, n_q, n_k, causal, scale, window, starts)
    return O[..., :D_V], L


@functools.lru_cache(maxsize=32)
def batch_reference(g, h_kv, dtype, causal, window):
    return reference(queries(g, h_kv, dtype), cache(h_kv, dtype), N_Q, N_K, causal, SCALE, window)


def check_forward(O, L, O_ref, L_ref, dtype, what):
    """the bars of tests/test_decode_gpu.py, L (H, total_q) viewed token-first as O's leading axes are"""
    check_bhn(O, L.t(), O_ref, L_ref.t(), dtype, what)


def call(Q, KV, n_q=N_Q, n_k=N_K, max_q=MAX_Q, **kw):
    kw.setdefault("scale", SCALE)
    return fa.flash_attention_mla_varlen_decode_forward(Q, KV, cu_of(n_q), max_q, lens_of(n_k), DEV, **kw)


CASES = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic")]


@gpu
@pytest.mark.parametrize("rotation,dtype,variant", [(k,) + c for k, c in enumerate(CASES)], ids=ids)
def test_forward_against_fp64_truth(rotation, dtype, variant):
    cfgs = [c + (SPLITS[(k + rotation) % len(SPLITS)],) for k, c in enumerate(CONFIGS)]
    assert {c[4] for c in cfgs} == set(SPLITS)
    for g, h_kv, causal, window, n in cfgs:
        Q, KV = queries(g, h_kv, dtype), cache(h_kv, dtype)
        O, L = call(Q, KV, causal=causal, window=window, num_splits=n, variant=variant)
        assert O.shape == (TOTAL, g * h_kv, D_V) and L.shape == (g * h_kv, TOTAL) and O.dtype == dtype and L.dtype == dtype
        assert O.is_contiguous()
        O_ref, L_ref = batch_reference(g, h_kv, dtype, causal, window)
        check_forward(O, L, O_ref, L_ref, dtype, (dtype, variant, g, h_kv, causal, window, n))


@gpu
@pytest.mark.parametrize("variant,g,h_kv,causal,window,n", [("mla16", 40, 1, True, None, 3), ("mla16", 128, 1, False, (100, 50), 1),
                                                            ("mla16", 16, 2, True, (64, 0), 7), ("generic", 5, 1, True, None, 2)], ids=ids)
def test_each_sequence_alone_equals_its_rows_in_the_batch(variant, g, h_kv, causal, window, n):
    """in bf16 and in f16 (the one-split case among them)"""
    for dtype in (BF16, F16):
        Q, KV = queries(g, h_kv, dtype), cache(h_kv, dtype)
        kw = dict(causal=causal, window=window, num_splits=n, variant=variant)
        O, L = call(Q, KV, **kw)
        O2, L2 = call(Q, KV, **kw)
        assert torch.equal(O, O2) and torch.equal(L, L2), dtype                         # the same call twice
        start = 0
        for b, (nq, nk) in enumerate(zip(N_Q, N_K)):
            if nq:
                Ob, Lb = call(Q[start:start + nq], KV[b:b + 1], [nq], [nk], nq, **kw)
                assert torch.equal(Ob, O[start:start + nq]) and torch.equal(Lb, L[:, start:start + nq]), (dtype, b, nq, nk)
            start += nq


@gpu
@pytest.mark.parametrize("cache_dtype", [None, E4M3], ids=ids)
@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("g,n_q", [(16, 1), (16, 2), (128, 1), (128, 2)])
def test_uniform_batch_equals_the_fixed_call_bit_for_bit(g, n_q, variant, cache_dtype):
    """in bf16 and in f16: at one split the f16 epilogue must round each product once, as the fixed kernel's does"""
    lens = [0, 1, 64, 65, 700, 1280, 3]
    nb = len(lens)
    for dtype in (BF16, F16):
        gen = torch.Generator().manual_seed(g + n_q)
        Q = (torch.randn(nb, g, n_q, D, generator=gen) * 0.5).to(dtype).to(DEV)
        KV = cache(1, dtype)[:nb, :, :1280]
        kd = None
        if cache_dtype is not None:
            KV, kd = fa.quantize_kv_cache(KV, cache_dtype)
        Qp = Q.transpose(1, 2).reshape(nb * n_q, g, D)
        for causal, window, n in ((False, None, 1), (True, None, 4), (False, (100, 50), 3), (True, (64, 0), 16)):
            kw = dict(causal=causal, window=window, scale=SCALE, num_splits=n, variant=variant, kv_descale=kd)
            O, L = fa.flash_attention_mla_decode_forward(Q, KV, lens_of(lens), DEV, **kw)
            Op, Lp = fa.flash_attention_mla_varlen_decode_forward(Qp, KV, cu_of([n_q] * nb), n_q, lens_of(lens), DEV, **kw)
            assert torch.equal(Op.view(nb, n_q, g, D_V).transpose(1, 2), O), (dtype, causal, window, n)
            assert torch.equal(Lp.view(g, nb, n_q).permute(1, 0, 2), L), (dtype, causal, window, n)


def scatter(KV, page, seed, n_k, fill=float("nan"), share=True):
    """the contiguous cache scattered into a pool under a seeded permutation table, five spare pages; the table entries of pages no
    key of the sequence lies in are -1 and 2^31 - 1, those pages and the spare ones hold `fill`, and so do the rows of a last page
    behind N_k(b).  share: sequences whose first page holds the rows of the first such sequence point at ONE page.  An fp8 cache
    goes through its uint8 view (fill 127: NaN in both formats) -> (pool, table)"""
    Bc, h_kv, s_k, d = KV.shape
    mb = s_k // page
    assert mb * page == s_k
    nb = Bc * mb + 5
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:Bc * mb].view(Bc, mb).clone()
    used = torch.arange(mb, device=DEV).view(1, mb) * page < torch.tensor(n_k, device=DEV).view(Bc, 1)
    t = KV.clone()
    for b, nk in enumerate(n_k):
        t[b, :, nk:] = fill
    pages = t.view(Bc, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(Bc * mb, h_kv, page, d)
    pool = torch.full((nb, h_kv, page, d), fill, dtype=KV.dtype, device=DEV)
    pool[table[used]] = pages[used.view(-1)]
    wild = torch.where((torch.arange(Bc * mb, device=DEV).view(Bc, mb) % 2) == 0, -1, 2 ** 31 - 1)
    table = torch.where(used, table, wild)
    if share:
        full = [b for b, nk in enumerate(n_k) if nk >= page]
        for b in full[1:]:
            if torch.equal(KV[b, :, :page], KV[full[0], :, :page]):
                table[b, 0] = table[full[0], 0]
    return pool, table.to(torch.int32).contiguous()


def scatter8(KV8, page, seed, n_k, **kw):
    pool, table = scatter(KV8.view(torch.uint8), page, seed, n_k, fill=127, **kw)
    return pool.view(KV8.dtype), table


@functools.lru_cache(maxsize=2)
def shared_prefix_cache(dtype):
    """the batch's cache with one 256-key prefix common to every sequence that long: their first page is then ONE pool page"""
    KV = cache(1, dtype).clone()
    for b, nk in enumerate(N_K):
        if nk >= 256:
            KV[b, :, :256] = KV[5, :, :256]
    return KV


@gpu
@pytest.mark.parametrize("page,variant,dtype,g", [(64, "mla16", BF16, 40), (256, "mla16", F16, 128), (256, "auto", BF16, 16),
                                                   (64, "generic", BF16, 5), (16, "generic", BF16, 16)], ids=ids)
def test_paged_pool_equals_the_contiguous_cache_bit_for_bit(page, variant, dtype, g):
    KV, Q = shared_prefix_cache(dtype), queries(g, 1, dtype)
    pool, table = scatter(KV, page, 11 * page + g, N_K)
    if page == 256:
        assert len({int(table[b, 0]) for b, nk in enumerate(N_K) if nk >= 256}) == 1    # shared pages
    t0, p0 = table.clone(), pool.clone()
    for causal, window, n in ((True, None, 3), (False, (100, 50), 1), (True, (64, 0), 16)):
        kw = dict(causal=causal, window=window, num_splits=n, variant=variant)
        O, L = call(Q, KV, **kw)
        Op, Lp = call(Q, pool, block_table=table, **kw)
        assert not torch.isnan(Op).any()
        assert torch.equal(Op, O) and torch.equal(Lp, L), (causal, window, n)
    assert torch.equal(table, t0) and torch.equal(pool.view(torch.int16), p0.view(torch.int16))
    if page == 16:  # no multiple of 64: "auto" is the VALU form, a forced matrix form refuses
        Oa, La = call(Q, pool, block_table=table, **dict(kw, variant="auto"))
        assert torch.equal(Oa, Op) and torch.equal(La, Lp)
        with pytest.raises(TypeError, match="page_size % 64"):
            call(Q, pool, block_table=table, **dict(kw, variant="mla16"))


@gpu
@pytest.mark.parametrize("cache_dtype", [E4M3, E5M2], ids=ids)
@pytest.mark.parametrize("variant,dtype,g", [("mla16", BF16, 40), ("mla16", F16, 128), ("generic", BF16, 16)], ids=ids)
def test_fp8_cache_without_descale_equals_the_converted_cache(variant, dtype, g, cache_dtype):
    KV8 = cache(1, dtype).to(cache_dtype)
    Q = queries(g, 1, dtype)
    for causal, window, n in ((True, None, 2), (False, (100, 50), 1), (True, (64, 0), 7)):
        kw = dict(causal=causal, window=window, num_splits=n, variant=variant)
        O8, L8 = call(Q, KV8, **kw)
        O, L = call(Q, KV8.to(dtype), **kw)
        assert torch.equal(O8, O) and torch.equal(L8, L), (causal, window, n)


@gpu
@pytest.mark.parametrize("cache_dtype", [E4M3, E5M2], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
def test_fp8_cache_with_descales_against_the_truth_on_the_dequantised_rows(variant, cache_dtype):
    dtype = BF16
    for k, (g, h_kv, causal, window) in enumerate(((16, 2, True, None), (128, 1, False, (100, 50)), (40, 1, True, (64, 0)))):
        KV = cache(h_kv, dtype) * (torch.arange(1, B + 1, device=DEV).view(B, 1, 1, 1) * 0.75).to(dtype)  # a descale per sequence
        KV8, kd = fa.quantize_kv_cache(KV, cache_dtype)
        assert kd.shape == (B, h_kv) and kd.unique().numel() > 1
        Q = queries(g, h_kv, dtype)
        n = SPLITS[(2 * k + 1) % len(SPLITS)]
        O, L = call(Q, KV8, causal=causal, window=window, num_splits=n, variant=variant, kv_descale=kd, scale=0.02)
        rows = KV8.float().double() * kd.double()[:, :, None, None]                              # exactly what the kernel is defined on
        O_ref, L_ref = reference(Q, rows, N_Q, N_K, causal, 0.02, window)
        check_forward(O, L, O_ref, L_ref, dtype, (variant, cache_dtype, g, h_kv, causal, window, n))


@gpu
@pytest.mark.parametrize("variant,dtype", [("mla16", BF16), ("mla16", F16), ("generic", BF16), ("generic", F32)], ids=ids)
def test_stale_rows_do_not_reach_the_output(variant, dtype):
    g = 40
    KV, Q = cache(1, dtype), queries(g, 1, dtype)
    for causal, window, n in ((True, None, 0), (False, (100, 50), 1), (True, (64, 0), 128)):
        outs = []
        for fill in (0.0, float("nan"), float("inf"), float("-inf")):
            KVf = KV.clone()
            for b, nk in enumerate(N_K):
                KVf[b, :, nk:] = fill
            outs.append(call(Q, KVf, causal=causal, window=window, num_splits=n, variant=variant))
        for O, L in outs[1:]:
            assert torch.equal(O, outs[0][0]) and torch.equal(L, outs[0][1]), (causal, window, n, fill)
        assert not torch.isnan(outs[0][0]).any() and not torch.isnan(outs[0][1]).any()


@gpu
@pytest.mark.parametrize("variant,dtype,cache_dtype", [("mla16", BF16, None), ("mla16", F16, E4M3), ("generic", BF16, None)], ids=ids)
def test_poison_canaries_and_rows_outside_every_sequence(variant, dtype, cache_dtype):
    """the entry point itself, on outputs and a workspace inside canary arenas.  cu_seqlens_q gives the 70-token sequence four rows
    more than max_seqlen_q and total_q runs three rows past the last sequence: those rows of O and L keep what they held.  A
    poisoned workspace (NaN, +-inf) does not change a bit, nothing outside O, L and the workspace is written, no input is modified,
    and the pool (unused pages NaN) gives the contiguous cache's bits."""
    g, page = 16, 64
    H = g
    enum = convert_triton_dtype(dtype)
    KV = cache(1, dtype) if cache_dtype is None else cache(1, dtype).to(cache_dtype)
    pool, table = scatter(KV, page, 5, N_K) if cache_dtype is None else scatter8(KV, page, 5, N_K)
    starts, s = [], 0
    for nq in N_Q:
        starts.append(s)
        s += nq + (4 if nq == MAX_Q else 0)
    total = s + 3
    cu = torch.tensor(starts + [s], dtype=torch.int32, device=DEV)
    live = torch.zeros(total, dtype=torch.bool, device=DEV)
    for st, nq in zip(starts, N_Q):
        live[st:st + nq] = True
    assert int((~live).sum()) == 7
    Q = (torch.randn(total, H, D, generator=torch.Generator().manual_seed(3)) * 0.5).to(dtype).to(DEV)
    lens = lens_of(N_K)
    O_ref, L_ref = reference(Q, KV.float(), N_Q, N_K, True, SCALE, None, starts)
    raw = lambda t: t.view(torch.uint8)
    before = [raw(t).clone() for t in (Q, KV, pool, table, cu, lens)]
    for n in (1, 5, 16):
        per_cache = []
        for paged in (False, True):
            results = []
            for poison in (0.0, float("nan"), float("inf"), float("-inf")):
                ws, ws_all, ws_sl = arena(max(_lib.kvcache_varlen_workspace_bytes(total, H, D_V, n) // 4, 16), F32, 77.0)
                ws.fill_(poison)
                O, O_all, O_sl = arena(total * H * D_V, dtype, 77.0)
                L, L_all, L_sl = arena(H * total, dtype, 77.0)
                O3, L2 = O.view(total, H, D_V), L.view(H, total)
                _lib.fa2_fwd_kvcache_mla_varlen(Q, pool if paged else KV, O3, L2, cu, MAX_Q, lens, enum, convert_triton_dtype(KV.dtype), D_V,
                                                block_table=table if paged else None, causal=True, scale=SCALE, num_splits=n,
                                                workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
                torch.cuda.synchronize()
                assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
                assert (O3[~live] == 77.0).all() and (L2[:, ~live] == 77.0).all(), (variant, n)  # rows outside every sequence
                if n == 1:
                    assert (ws == poison).all() or torch.isnan(ws).all()                       # not touched
                results.append((O3.clone(), L2.clone()))
            for O3, L2 in results[1:]:
                assert torch.equal(O3, results[0][0]) and torch.equal(L2, results[0][1]), (variant, n, paged)
            per_cache.append(results[0])
        (O3, L2), (Op, Lp) = per_cache
        assert torch.equal(Op, O3) and torch.equal(Lp, L2), (variant, n)
        check_forward(O3[live], L2[:, live], O_ref[live], L_ref[:, live], dtype, ("gaps", dtype, variant, n))
    for t, t0 in zip((Q, KV, pool, table, cu, lens), before):
        assert torch.equal(raw(t), t0)


@gpu
@pytest.mark.parametrize("cache_dtype,paged,causal,interleaved,pair,variant",
                         [(None, False, True, False, False, "mla16"), (None, True, False, True, True, "mla16"),
                          (E4M3, True, True, False, True, "mla16"), (E5M2, False, False, True, False, "auto"),
                          (None, True, True, True, False, "generic")], ids=ids)
def test_fused_step_equals_the_append_followed_by_the_attention(cache_dtype, paged, causal, interleaved, pair, variant):
    dtype, g, page, rd = BF16, 40, 64, 64
    gen = torch.Generator().manual_seed(23)
    before = N_K  # the lengths BEFORE the append; the token of the sequence that fills its cache is dropped
    KV = cache(1, dtype).clone()
    kd = None
    if cache_dtype is not None:
        KV, kd = fa.quantize_kv_cache(KV, cache_dtype)
    table = None
    if paged:
        KV, table = (scatter8 if cache_dtype else scatter)(KV, page, 7, [S_K] * B, share=False)
    Q = queries(g, 1, dtype)
    new = (torch.randn(TOTAL, 1, D, generator=gen) * 0.5).to(dtype).to(DEV)
    kv_new = (new[..., :D_V], new[..., D_V:].clone()) if pair else new
    cos = torch.cos(torch.rand(S_K + 8, rd // 2, generator=gen) * 6.28).to(dtype).to(DEV)
    sin = torch.sin(torch.rand(S_K + 8, rd // 2, generator=gen) * 6.28).to(dtype).to(DEV)
    lens, cu = lens_of(before), cu_of(N_Q)
    for n in (1, 3):
        common = dict(causal=causal, scale=SCALE, block_table=table, kv_descale=kd, num_splits=n, variant=variant)
        KV1, KV2 = KV.clone(), KV.clone()
        O1, L1 = fa.flash_attention_mla_varlen_decode_forward(Q, KV1, cu, MAX_Q, lens, DEV, kv_new=kv_new, rotary_cos=cos, rotary_sin=sin,
                                                              rotary_interleaved=interleaved, **common)
        new_lens = fa.mla_kvcache_append_varlen(KV2, kv_new, cu, MAX_Q, lens, kv_descale=kd, block_table=table, rotary_cos=cos,
                                                rotary_sin=sin, rotary_interleaved=interleaved)
        pos = torch.cat([torch.full((nq,), s, dtype=torch.long) + (torch.arange(nq) if causal else 0) for nq, s in zip(N_Q, before)])
        Qr = Q.clone()
        Qr[..., D_V:] = fa.apply_rotary(Q[..., D_V:], cos, sin, pos.to(DEV)[:, None], interleaved)
        O2, L2 = fa.flash_attention_mla_varlen_decode_forward(Qr, KV2, cu, MAX_Q, new_lens, DEV, **common)
        assert new_lens.tolist() == [min(s + nq, S_K) for nq, s in zip(N_Q, before)]
        assert torch.equal(lens, lens_of(before))                                        # the lengths before the append are not modified
        assert torch.equal(KV1.view(torch.uint8), KV2.view(torch.uint8)), n              # the cache bytes are the append's
        assert not torch.equal(KV1.view(torch.uint8), KV.view(torch.uint8))
        assert torch.isfinite(O1.float()).all()
        assert torch.equal(O1, O2) and torch.equal(L1, L2), n


@gpu
def test_strided_and_misaligned_queries():
    g, dtype = 16, BF16
    KV, Q = cache(1, dtype), queries(g, 1, dtype)
    kw = dict(causal=True, num_splits=3)
    O, L = call(Q, KV, variant="mla16", **kw)
    # a slice of a wider tensor: token, head and column strides of its own, rows still 16-byte aligned
    wide = torch.zeros(TOTAL, g + 3, D + 64, dtype=dtype, device=DEV)
    Qs = wide[:, 2:2 + g, 8:8 + D]
    Qs.copy_(Q)
    assert not Qs.is_contiguous() and Qs.data_ptr() % 16 == 0
    Os, Ls = call(Qs, KV, variant="mla16", **kw)
    assert torch.equal(Os, O) and torch.equal(Ls, L)
    # one element off the 16-byte grid: "auto" is the VALU form, a forced matrix form refuses
    Qm = wide[:, 2:2 + g, 9:9 + D]
    Qm.copy_(Q)
    assert Qm.data_ptr() % 16 != 0
    Oa, La = call(Qm, KV, variant="auto", **kw)
    Og, Lg = call(Q, KV, variant="generic", **kw)
    assert torch.equal(Oa, Og) and torch.equal(La, Lg)
    check_forward(Oa, La, *batch_reference(g, 1, dtype, True, None), dtype, "misaligned Q on auto")
    with pytest.raises(TypeError, match="16-byte"):
        call(Qm, KV, variant="mla16", **kw)
