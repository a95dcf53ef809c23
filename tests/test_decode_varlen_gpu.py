"""Variable-length (packed) queries over the KV cache (fa2_fwd_kvcache_varlen) on the GPU, one ragged batch whose sequences bring
0 to 300 query tokens over caches of 0 to 2560 keys: O and L against the fp64 per-sequence truth at the bars of
tests/test_decode_gpu.py for both kernel forms, every dtype, group size, mask and split count; bit-identities (paged against
contiguous, fp8 at descale 1 against the converted cache, every sequence alone against its rows in the batch, the uniform batch
against flash_attention_kvcache_forward, the same call twice); stale rows, unused pages and a poisoned workspace that must not
reach the output; canaries around O, L and the workspace, rows outside every sequence untouched, inputs unchanged; forced-variant
rejections; strided layouts."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_bwd_arith
from test_decode_gpu import arena, canaries_intact, f32, lens_of
from test_decode_gpu import check_forward as check_bhn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64

S_K = 2560
H_KV = 2
MAX_Q = 300
N_Q = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130, 1, 300]
N_K = [100, 0, 2, 16, 10, 65, 1000, 64, S_K, 200, 777, 2500]
B = len(N_Q)
SPLITS = (0, 1, 2, 3, 7, 16, 128)
WINDOWS = (None, (64, 0), (100, 50), (0, 0))
# (g, causal, window): every group size of the matrix form, every window, causal on and off; the split counts rotate over them
CONFIGS = [(1, True, None), (3, False, (64, 0)), (4, True, (100, 50)), (8, False, None), (32, True, (0, 0)), (64, False, (100, 50)),
           (4, True, (64, 0)), (64, True, None)]
VALU_CONFIG = (128, True, None)  # g > 64: the VALU form only

ids = lambda x: str(x).replace("torch.", "")


def cu_of(n_q):
    return torch.tensor([0] + torch.tensor(list(n_q)).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def split_chunk(n_k, num_splits):
    return ((n_k + num_splits - 1) // num_splits + 63) & ~63


def test_the_batch_holds_every_class_of_length():
    pairs = list(zip(N_Q, N_K))
    assert any(nq > 0 and nk == 0 for nq, nk in pairs)                                  # N_k = 0
    assert any(0 < nk < nq for nq, nk in pairs)                                         # N_k < n_q: rows without a key under causal
    assert sum(nq > 0 and nk == nq for nq, nk in pairs) >= 2                            # pure prefill, one of them a whole key tile
    assert any(nk == nq + 1 for nq, nk in pairs)
    assert any(nk > nq > 0 and (nk - nq) // 64 != (nk - 1) // 64 for nq, nk in pairs)   # the chunk straddles a 64-key tile edge
    assert any(nk == S_K for nk in N_K) and any(nq == 0 for nq in N_Q) and max(N_Q) == MAX_Q
    for n in SPLITS[2:]:                                                                # ... and a split edge, at every split count
        assert any(nk - nq < s * split_chunk(nk, n) < nk for nq, nk in pairs if nq > 1 for s in range(1, n)), n


@functools.lru_cache(maxsize=8)
def cache(d, dtype, seed=1):
    g = torch.Generator().manual_seed(seed + d)
    K = (torch.randn(B, H_KV, S_K, d, generator=g) * 0.5).to(dtype).to(DEV)
    V = (torch.randn(B, H_KV, S_K, d, generator=g) * 0.5).to(dtype).to(DEV)
    return K, V


@functools.lru_cache(maxsize=32)
def queries(g, d, dtype, total=sum(N_Q)):
    gen = torch.Generator().manual_seed(7 * d + g)
    return (torch.randn(total, g * H_KV, d, generator=gen) * 0.5).to(dtype).to(DEV)


def reference(Q, K, V, n_q, n_k, causal, scale, window, starts=None):
    """fp64 truth, one sequence at a time, over the first N_k(b) keys with the band of its own n_q(b): O (total_q, H, d),
    L (H, total_q); rows without a visible key get O = 0 and L = +inf (rows outside every sequence as well)."""
    total, H, d = Q.shape
    g = H // K.shape[1]
    O = torch.zeros(total, H, d, dtype=F64, device=DEV)
    L = torch.full((H, total), math.inf, dtype=F64, device=DEV)
    start = 0
    for b, (nq, nk) in enumerate(zip(n_q, n_k)):
        s = start if starts is None else starts[b]
        start += nq
        if nq == 0 or nk == 0:
            continue
        m = fa2_bwd_arith.band(nq, nk, causal, window, DEV)
        vis = m.any(-1)
        for hk in range(K.shape[1]):
            hs = slice(hk * g, (hk + 1) * g)
            q, k, v = Q[s:s + nq, hs].double().transpose(0, 1), K[b, hk, :nk].double(), V[b, hk, :nk].double()
            S = ((q @ k.T) * f32(scale)).masked_fill(~m, float("-inf"))
            P = torch.where(vis.view(nq, 1), torch.softmax(S.masked_fill(~vis.view(nq, 1), 0.0), -1), 0.0)
            O[s:s + nq, hs] = (P @ v).transpose(0, 1)
            L[hs, s:s + nq] = torch.where(vis, torch.logsumexp(S, -1) * math.log2(math.e), math.inf)
    return O, L


@functools.lru_cache(maxsize=32)
def batch_reference(g, d, dtype, causal, window):
    K, V = cache(d, dtype)
    return reference(queries(g, d, dtype), K, V, N_Q, N_K, causal, 1.0 / math.sqrt(d), window)


def check_forward(O, L, O_ref, L_ref, dtype, what):
    """the bars of tests/test_decode_gpu.py, L (H, total_q) viewed token-first as O's leading axes are"""
    check_bhn(O, L.t(), O_ref, L_ref.t(), dtype, what)


def call(Q, K, V, n_q=N_Q, n_k=N_K, max_q=MAX_Q, **kw):
    return fa.flash_attention_varlen_kvcache_forward(Q, K, V, cu_of(n_q), max_q, lens_of(n_k), DEV, **kw)


CASES = [(dt, v, d) for dt in (F16, BF16) for v in ("auto", "generic", "mfma16") for d in (64, 128)]
CASES += [(dt, v, d) for dt in (F32, F64) for v in ("auto", "generic") for d in (64, 40)]


@pytest.mark.parametrize("rotation,dtype,variant,d", [(k,) + c for k, c in enumerate(CASES)], ids=ids)
def test_forward_against_fp64_truth(rotation, dtype, variant, d):
    cfgs = CONFIGS + ([VALU_CONFIG] if variant != "mfma16" else [])
    assert {c[0] for c in CONFIGS} == {1, 3, 4, 8, 32, 64} and {c[2] for c in CONFIGS} == set(WINDOWS)
    assert {c[1] for c in CONFIGS} == {False, True}
    cfgs = [c + (SPLITS[(k + rotation) % len(SPLITS)],) for k, c in enumerate(cfgs)]
    assert {c[3] for c in cfgs} == set(SPLITS)
    K, V = cache(d, dtype)
    for g, causal, window, n in cfgs:
        Q = queries(g, d, dtype)
        O, L = call(Q, K, V, causal=causal, scale=1.0 / math.sqrt(d), window=window, num_splits=n, variant=variant)
        assert O.shape == Q.shape and L.shape == (g * H_KV, Q.shape[0]) and O.dtype == dtype and L.dtype == dtype
        O_ref, L_ref = batch_reference(g, d, dtype, causal, window)
        check_forward(O, L, O_ref, L_ref, dtype, (dtype, variant, d, g, causal, window, n))


SPARE = 5


def scatter(K, V, page, seed, n_k, fill=float("nan")):
    """the contiguous cache scattered into pools of B * max_blocks + SPARE pages under a seeded permutation table; the table entries
    of pages no key of the sequence lies in are -1 and 2^31 - 1, those pages and the spare ones hold `fill`, and so do the rows of
    a last page behind N_k(b) -> (K_pool, V_pool, table)"""
    Bc, h_kv, s_k, d = K.shape
    mb = s_k // page
    assert mb * page == s_k
    nb = Bc * mb + SPARE
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:Bc * mb].view(Bc, mb).clone()
    used = torch.arange(mb, device=DEV).view(1, mb) * page < torch.tensor(n_k, device=DEV).view(Bc, 1)
    pools = []
    for t in (K, V):
        t = t.clone()
        for b, nk in enumerate(n_k):
            t[b, :, nk:] = fill
        pages = t.view(Bc, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(Bc * mb, h_kv, page, d)
        pool = torch.full((nb, h_kv, page, d), fill, dtype=t.dtype, device=DEV)
        pool[table[used]] = pages[used.view(-1)]
        pools.append(pool)
    wild = torch.where((torch.arange(Bc * mb, device=DEV).view(Bc, mb) % 2) == 0, -1, 2 ** 31 - 1)
    table = torch.where(used, table, wild)
    return pools[0], pools[1], table.to(torch.int32).contiguous()


PAGED = [(64, "mfma16", BF16, 128, 8), (128, "mfma16", F16, 64, 3), (16, "generic", BF16, 64, 4), (16, "auto", F32, 40, 4),
         (64, "auto", BF16, 64, 64)]


@pytest.mark.parametrize("page,variant,dtype,d,g", PAGED, ids=ids)
def test_paged_pool_equals_the_contiguous_cache_bit_for_bit(page, variant, dtype, d, g):
    K, V = cache(d, dtype)
    Q = queries(g, d, dtype)
    Kp, Vp, table = scatter(K, V, page, 11 * page + d, N_K)
    t0 = table.clone()
    for causal, window, n in ((True, None, 3), (False, (100, 50), 1), (True, (64, 0), 16)):
        kw = dict(causal=causal, scale=0.1, window=window, num_splits=n, variant=variant)
        O, L = call(Q, K, V, **kw)
        Op, Lp = call(Q, Kp, Vp, block_table=table, **kw)
        assert not torch.isnan(Op).any() and not torch.isnan(Lp).any()
        assert torch.equal(O, Op) and torch.equal(L, Lp), (page, variant, causal, window, n)
    assert torch.equal(table, t0)


@pytest.mark.parametrize("fmt", [torch.float8_e4m3fn, torch.float8_e5m2], ids=ids)
@pytest.mark.parametrize("dtype,variant,d", [(BF16, "mfma16", 128), (F16, "mfma16", 64), (BF16, "generic", 64)], ids=ids)
def test_fp8_cache_at_descale_one_equals_the_converted_cache_bit_for_bit(fmt, dtype, variant, d):
    K, V = cache(d, dtype)
    K8, V8 = (K.float() * 4).to(fmt), (V.float() * 4).to(fmt)
    K16, V16 = K8.to(dtype), V8.to(dtype)
    ones = torch.ones(B, H_KV, device=DEV)
    Q = queries(4, d, dtype)
    for causal, window, n in ((True, None, 2), (False, (64, 0), 1), (True, (100, 50), 7)):
        kw = dict(causal=causal, scale=0.05, window=window, num_splits=n, variant=variant)
        O, L = call(Q, K16, V16, **kw)
        O8, L8 = call(Q, K8, V8, k_descale=ones, v_descale=ones, **kw)
        assert torch.equal(O, O8) and torch.equal(L, L8), (fmt, variant, causal, window, n)
        O8, L8 = call(Q, K8, V8, **kw)  # no descales: 1
        assert torch.equal(O, O8) and torch.equal(L, L8)


@pytest.mark.parametrize("dtype,variant,d,g,causal,window,n", [(BF16, "mfma16", 128, 4, True, None, 3),
                                                               (F16, "mfma16", 64, 32, True, (100, 50), 1),
                                                               (BF16, "generic", 64, 3, True, (64, 0), 2),
                                                               (F32, "auto", 40, 1, False, None, 7)], ids=ids)
def test_every_sequence_alone_equals_its_rows_in_the_batch(dtype, variant, d, g, causal, window, n):
    K, V = cache(d, dtype)
    Q = queries(g, d, dtype)
    kw = dict(causal=causal, scale=0.1, window=window, num_splits=n, variant=variant)
    O, L = call(Q, K, V, **kw)
    cu = [0] + list(torch.tensor(N_Q).cumsum(0).tolist())
    for b, (nq, nk) in enumerate(zip(N_Q, N_K)):
        if nq == 0:
            continue
        rows = slice(cu[b], cu[b + 1])
        Ob, Lb = call(Q[rows], K[b:b + 1], V[b:b + 1], [nq], [nk], **kw)
        assert torch.equal(Ob, O[rows]) and torch.equal(Lb, L[:, rows]), (b, nq, nk)


@pytest.mark.parametrize("g,n_q", [(4, 1), (8, 5), (1, 16), (32, 2)])
@pytest.mark.parametrize("dtype,variant,d", [(BF16, "mfma16", 128), (F16, "mfma16", 64), (BF16, "generic", 64)], ids=ids)
def test_uniform_batch_equals_the_fixed_call_bit_for_bit(g, n_q, dtype, variant, d):
    """n_q(b) = max_seqlen_q = N_q with g N_q <= 64: the tile, the row order and the key groups are the fixed-N_q kernel's"""
    lens = [0, 1, 63, 700, S_K, 5, 129]
    Bu, H = len(lens), g * H_KV
    K, V = (t[:Bu] for t in cache(d, dtype))
    Q = queries(g, d, dtype, total=Bu * n_q)
    Q4 = Q.view(Bu, n_q, H, d).transpose(1, 2)
    for causal, window, n in ((False, None, 1), (True, None, 4), (True, (64, 0), 128), (False, (100, 50), 3)):
        kw = dict(causal=causal, scale=0.1, window=window, num_splits=n, variant=variant)
        O4, L3 = fa.flash_attention_kvcache_forward(Q4, K, V, lens_of(lens), DEV, **kw)
        O, L = call(Q, K, V, [n_q] * Bu, lens, n_q, **kw)
        assert torch.equal(O.view(Bu, n_q, H, d).transpose(1, 2), O4), (g, n_q, causal, window, n)
        assert torch.equal(L.view(H, Bu, n_q).transpose(0, 1), L3), (g, n_q, causal, window, n)


@pytest.mark.parametrize("dtype,variant,page", [(BF16, "mfma16", None), (BF16, "mfma16", 64), (F16, "generic", None), (BF16, "generic", 16),
                                                (F32, "auto", None)], ids=ids)
def test_stale_rows_and_unused_pages_do_not_reach_the_output(dtype, variant, page):
    d, g = 64, 4
    K, V = cache(d, dtype)
    Q = queries(g, d, dtype)
    for causal, window, n in ((True, None, 1), (False, (100, 50), 4), (True, None, 128)):
        outs = []
        for fill in (0.0, float("nan"), float("inf"), float("-inf")):
            kw = dict(causal=causal, scale=0.1, window=window, num_splits=n, variant=variant)
            if page:
                Kf, Vf, table = scatter(K, V, page, 3, N_K, fill)
                kw["block_table"] = table
            else:
                Kf, Vf = K.clone(), V.clone()
                for b, nk in enumerate(N_K):
                    Kf[b, :, nk:] = fill
                    Vf[b, :, nk:] = fill
            outs.append(call(Q, Kf, Vf, **kw))
        for O, L in outs[1:]:
            assert not torch.isnan(O).any() and not torch.isnan(L).any()
            assert torch.equal(O, outs[0][0]) and torch.equal(L, outs[0][1]), (causal, window, n)


@pytest.mark.parametrize("dtype,variant,page", [(BF16, "mfma16", None), (BF16, "mfma16", 64), (BF16, "generic", 16), (F32, "generic", None)],
                         ids=ids)
def test_workspace_poison_canaries_gap_rows_and_inputs(dtype, variant, page):
    """cu_seqlens_q gives one sequence more rows than max_seqlen_q and total_q runs past the last sequence: the surplus and the
    trailing rows of O and L keep their canary, with one split and through the combine launch"""
    H, d, max_q = 8, 64, 64
    g = H // H_KV
    n_cu = [3, 0, 100, 17, 64]          # rows per cu_seqlens_q; sequence 2 runs 64 of its 100
    n_q = [min(n, max_q) for n in n_cu]
    n_k = [300, 50, 1000, 10, 64]
    Bc, tail = len(n_cu), 7
    cu = cu_of(n_cu)
    starts = cu[:-1].tolist()
    total = sum(n_cu) + tail
    live = torch.zeros(total, dtype=torch.bool, device=DEV)
    for s, n in zip(starts, n_q):
        live[s:s + n] = True
    assert int((~live).sum()) == 36 + tail
    K, V = (t[:Bc, :, :1024] for t in cache(d, dtype))
    kw = {}
    if page:
        K, V, table = scatter(K.contiguous(), V.contiguous(), page, 5, n_k, 0.0)
        kw["block_table"] = table
    Q = queries(g, d, dtype, total=total)
    lens = lens_of(n_k)
    enum = convert_triton_dtype(dtype)
    before = [t.clone() for t in (Q, K, V, cu, lens) + ((kw["block_table"],) if page else ())]
    Kc, Vc = (t[:Bc, :, :1024] for t in cache(d, dtype))
    O_ref, L_ref = reference(Q, Kc, Vc, n_q, n_k, True, 0.1, None, starts)
    for n in (1, 4, 128):
        words = max(_lib.kvcache_varlen_workspace_bytes(total, H, d, n) // 4, 64)
        assert n == 1 or words == n * total * H * (d + 1)
        results = []
        for poison in (0.0, float("nan"), float("nan")):
            O, O_all, O_sl = arena(total * H * d, dtype, 77.0)
            L, L_all, L_sl = arena(H * total, dtype, 77.0)
            ws, ws_all, ws_sl = arena(words, F32, 77.0)
            ws.fill_(poison)
            O3, L2 = O.view(total, H, d), L.view(H, total)
            _lib.fa2_fwd_kvcache_varlen(Q, K, V, O3, L2, cu, max_q, lens, enum, enum, causal=True, scale=0.1, num_splits=n, workspace=ws,
                                        variant=_lib.KVCACHE_VARIANTS[variant], **kw)
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
            assert (O3[~live] == 77.0).all() and (L2[:, ~live] == 77.0).all(), (variant, n)     # rows outside every sequence
            if n == 1:
                assert (ws == poison).all() or torch.isnan(ws).all()                          # not touched
            results.append((O3.clone(), L2.clone()))
        for O3, L2 in results[1:]:  # NaN-poisoned == zeroed workspace, and the same call twice
            assert torch.equal(O3, results[0][0]) and torch.equal(L2, results[0][1]), (variant, n)
        O3, L2 = results[0]
        check_forward(O3[live], L2[:, live], O_ref[live], L_ref[:, live], dtype, ("gaps", dtype, variant, page, n))
    for t, t0 in zip((Q, K, V, cu, lens) + ((kw["block_table"],) if page else ()), before):
        assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8))


def test_forced_mfma16_rejections_and_auto_runs_them():
    n_q, n_k = [5, 0, 40], [300, 77, 40]
    for dtype, d, H, H_kv, page in ((BF16, 64, 65, 1, None), (F32, 64, 8, 2, None), (BF16, 40, 8, 2, None), (BF16, 64, 8, 2, 16)):
        gen = torch.Generator().manual_seed(41)
        Q = (torch.randn(sum(n_q), H, d, generator=gen) * 0.5).to(dtype).to(DEV)
        K = (torch.randn(3, H_kv, 320, d, generator=gen) * 0.5).to(dtype).to(DEV)
        V = (torch.randn(3, H_kv, 320, d, generator=gen) * 0.5).to(dtype).to(DEV)
        kw = {}
        Kx, Vx = K, V
        if page:
            Kx, Vx, kw["block_table"] = scatter(K, V, page, 9, n_k, 0.0)
        with pytest.raises(TypeError):  # FA2_ERR_UNSUPPORTED
            call(Q, Kx, Vx, n_q, n_k, 40, variant="mfma16", **kw)
        O, L = call(Q, Kx, Vx, n_q, n_k, 40, causal=True, scale=0.1, num_splits=2, **kw)
        check_forward(O, L, *reference(Q, K, V, n_q, n_k, True, 0.1, None), dtype, ("auto", dtype, d, H, H_kv, page))


@pytest.mark.parametrize("dtype,variant", [(BF16, "mfma16"), (BF16, "generic"), (F32, "auto")], ids=ids)
def test_strided_queries_outputs_and_the_flash_attn_cache_layout(dtype, variant):
    d, g = 128, 4
    H = g * H_KV
    K, V = cache(d, dtype)
    Q = queries(g, d, dtype)
    total = Q.shape[0]
    bshd = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)  # (B, S, H_kv, d) storage, (B, H_kv, S, d) view
    Qs = Q.transpose(0, 1).contiguous().transpose(0, 1)            # (H, total_q, d) storage viewed as packed
    assert Qs.stride() == (d, total * d, 1) and bshd(K).stride(2) == H_KV * d
    enum = convert_triton_dtype(dtype)
    O_ref, L_ref = batch_reference(g, d, dtype, True, None)
    for n in (1, 3):
        O, L = call(Qs, bshd(K), bshd(V), causal=True, scale=1.0 / math.sqrt(d), num_splits=n, variant=variant)
        check_forward(O, L, O_ref, L_ref, dtype, ("strided Q, bshd cache", dtype, variant, n))
        Ob = torch.full((H, total, d), 77.0, dtype=dtype, device=DEV)
        Lb = torch.empty(H, total, dtype=dtype, device=DEV)
        ws = torch.empty(_lib.kvcache_varlen_workspace_bytes(total, H, d, n) // 4 + 4, dtype=F32, device=DEV)
        _lib.fa2_fwd_kvcache_varlen(Qs, bshd(K), bshd(V), Ob.transpose(0, 1), Lb, cu_of(N_Q), MAX_Q, lens_of(N_K), enum, enum, causal=True,
                                    scale=1.0 / math.sqrt(d), num_splits=n, workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
        assert torch.equal(Ob.transpose(0, 1), O) and torch.equal(Lb, L), (variant, n)
