"""Sparse MLA decode of packed queries (fa2_fwd_kvcache_mla_sparse_varlen) on the GPU.  The yardstick is the fixed call, which is
tested on its own: a workgroup's arithmetic for one token does not depend on how the tokens are packed, so O and L of a packed call
equal, BIT FOR BIT at an explicit and equal num_splits, the fixed call run per sequence on that sequence's slice.  Compared as integer
views, so NaN and -0.0 count; no tolerance enters.  Also: a uniform batch against the fixed batched call, paged against the same
fixed results at page sizes 1, 16, 48 and 64, rows no list names (and rows behind N_k(b)) and the workspace filled with NaN / inf,
canary arenas round O, L and the workspace -- under malformed cu_seqlens_q as well --, rows no sequence owns left unwritten, and the
fp64 truth of tests/test_decode_mla_sparse_gpu.py under check_forward's bars.  Both sides of these identities run the same row
expressions, on random data: tests/test_decode_mla_sparse_varlen_probe_gpu.py pins which sequence, list and keys each packed row reads,
to one output ulp."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import arena, canaries_intact, check_forward, lens_of
from test_decode_mla_sparse_gpu import paged, sparse_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
# the ragged batch: a sequence without a token, a sequence without a key, all lengths different (a row given the wrong sequence shows)
NQ = [3, 0, 1, 5, 2]
LENS = [200, 50, 0, 640, 65]
B, S_K, MAX_Q, TOTAL = len(NQ), 640, max(NQ), sum(NQ)
CU = [0, 3, 3, 4, 9, 11]
HEADS = [(16, 1), (128, 1), (32, 2)]  # (H, H_kv): one head tile, two head tiles, two KV heads with lists of their own
TOPKS = (64, 130)                     # whole tiles, and a partial last tile
SPLITS = (1, 3, 16)
SCALE = 576 ** -0.5
MLA = _lib.KVCACHE_MLA_VARIANTS
FORMS = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic")]
ids = lambda x: str(x).replace("torch.", "")


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def cu_of(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def starts(nq):
    out = [0]
    for n in nq:
        out.append(out[-1] + n)
    return out


def lists(H_kv, topk, seed, nq=NQ, lens=LENS):
    """int32 (total_q, H_kv, topk): per (row, KV head) distinct valid positions of the row's OWN sequence in shuffled order, mixed with
    -1, N_k(b), 2^31 - 1 and -2^31 (about one slot in five, and every slot a short sequence cannot fill)"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for n, nk in zip(nq, lens):
        for _ in range(n):
            per_head = []
            for _ in range(H_kv):
                junk = torch.tensor([-1, nk, 2 ** 31 - 1, -2 ** 31])[torch.randint(0, 4, (topk,), generator=g)]
                valid = torch.randperm(nk, generator=g)[:topk]
                slots = (torch.rand(topk, generator=g) < 0.8).nonzero().flatten()[:valid.numel()]
                junk[slots] = valid[:slots.numel()]
                per_head.append(junk)
            rows.append(torch.stack(per_head))
    return torch.stack(rows).to(torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs(dtype, H, H_kv, cache=None, seed=0, nq=tuple(NQ)):
    """packed Q (total_q, H, 576), the latent cache (B, H_kv, S_K, 576) in `cache` (None: dtype) and its descale"""
    g = torch.Generator().manual_seed(100 * H + H_kv + seed)
    Q = (torch.randn(sum(nq), H, 576, generator=g) * 0.5).to(dtype).to(DEV)
    KV = (torch.randn(len(nq), H_kv, S_K, 576, generator=g) * 0.5).to(dtype).to(DEV)
    kvd = None
    if cache is not None:
        KV, kvd = fa.quantize_kv_cache(KV, cache)
    return Q, KV, kvd


def fixed_per_sequence(Q, KV, kvd, idx, variant, n, nq=NQ, lens=LENS):
    """the fixed call on each sequence's slice -> packed (O, L); rows of a sequence without tokens do not exist"""
    total, H, _ = Q.shape
    O = torch.empty(total, H, 512, dtype=Q.dtype, device=DEV)
    L = torch.empty(H, total, dtype=Q.dtype, device=DEV)
    st = starts(nq)
    for b, cnt in enumerate(nq):
        if cnt == 0:
            continue
        s, e = st[b], st[b + 1]
        Ob, Lb = fa.flash_attention_mla_sparse_decode_forward(
            Q[s:e].transpose(0, 1)[None], KV[b:b + 1], idx[s:e].transpose(0, 1)[None], lens_of(lens[b:b + 1]), DEV, scale=SCALE, num_splits=n,
            variant=variant, kv_descale=None if kvd is None else kvd[b:b + 1])
        O[s:e] = Ob[0].transpose(0, 1)
        L[:, s:e] = Lb[0]
    return O, L


@functools.lru_cache(maxsize=None)
def fixed_case(dtype, H, H_kv, cache, topk, n, matrix):
    """the yardstick of one configuration, computed once and shared (auto and mla16 are the same kernel; the paged test reads it too)"""
    Q, KV, kvd = inputs(dtype, H, H_kv, cache)
    idx = lists(H_kv, topk, 7 * H + topk)
    return idx, fixed_per_sequence(Q, KV, kvd, idx, "mla16" if matrix else "generic", n)


@pytest.mark.parametrize("H,H_kv", HEADS)
@pytest.mark.parametrize("dtype,variant,cache", [(dt, v, c) for dt, v in FORMS for c in ((None,) if dt == F32 else (None, E4, E5))], ids=ids)
def test_ragged_batch_equals_the_fixed_call_per_sequence_bit_for_bit(dtype, variant, cache, H, H_kv):
    """(an fp8 cache goes with 16-bit Q: f32 runs over its own dtype alone)"""
    Q, KV, kvd = inputs(dtype, H, H_kv, cache)
    for topk in TOPKS:
        for n in SPLITS:
            idx, (O_fix, L_fix) = fixed_case(dtype, H, H_kv, cache, topk, n, variant != "generic")
            if H_kv == 2:
                assert not torch.equal(idx[:, 0], idx[:, 1])
            O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx, cu_of(CU), MAX_Q, lens_of(LENS), DEV, scale=SCALE,
                                                                       num_splits=n, variant=variant, kv_descale=kvd)
            assert O.shape == (TOTAL, H, 512) and L.shape == (H, TOTAL) and O.dtype == dtype and L.dtype == dtype
            assert not torch.isnan(O.float()).any()
            assert torch.isinf(L[:, 3]).all() and (O[3] == 0).all()  # the row of the sequence without a key
            assert same_bits(O, O_fix) and same_bits(L, L_fix), (dtype, variant, H, H_kv, cache, topk, n)


@pytest.mark.parametrize("page", [1, 16, 48, 64])
@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("cache", [None, E5], ids=ids)
def test_paged_equals_the_fixed_call_bit_for_bit(cache, variant, page):
    """a shuffled table; spare pages, and the tail of a last page at page size 48, hold NaN"""
    H, H_kv, topk = 32, 2, 130
    Q, KV, kvd = inputs(BF16, H, H_kv, cache)
    pool, table = paged(KV, page, 33 + page, fill=math.nan)
    assert torch.isnan(pool.float()).any() and not torch.equal(table.flatten(), torch.arange(table.numel(), dtype=torch.int32, device=DEV))
    for n in (1, 3):
        idx, (O_fix, L_fix) = fixed_case(BF16, H, H_kv, cache, topk, n, variant != "generic")
        O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, pool, idx, cu_of(CU), MAX_Q, lens_of(LENS), DEV, scale=SCALE, num_splits=n,
                                                                   variant=variant, kv_descale=kvd, block_table=table)
        assert not torch.isnan(O.float()).any() and same_bits(O, O_fix) and same_bits(L, L_fix), (cache, variant, page, n)


@pytest.mark.parametrize("N_q", [1, 2])
@pytest.mark.parametrize("dtype,variant", [(BF16, "mla16"), (F16, "mla16"), (BF16, "generic"), (F32, "generic")], ids=ids)
def test_uniform_batch_equals_the_fixed_batched_call_bit_for_bit(dtype, variant, N_q):
    """cu_seqlens_q = arange * N_q: the packed call is the fixed call on (B, H, N_q, d), also under the two heuristics (num_splits 0)"""
    H, topk = 128, 130
    nq = (N_q,) * B
    Q, KV, _ = inputs(dtype, H, 1, None, seed=N_q, nq=nq)
    idx = lists(1, topk, 5 + N_q, nq=nq)
    cu = cu_of([N_q * b for b in range(B + 1)])
    enum = convert_triton_dtype(dtype)
    assert _lib.kvcache_mla_sparse_varlen_num_splits(B * N_q, H, 1, topk, 576, 512, enum) == _lib.kvcache_mla_sparse_num_splits(B, H, 1, N_q, topk, 576, 512, enum)
    Q4 = Q.view(B, N_q, H, 576).permute(0, 2, 1, 3)
    idx4 = idx.view(B, N_q, 1, topk).permute(0, 2, 1, 3)
    for n in (0,) + SPLITS:
        O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx, cu, N_q, lens_of(LENS), DEV, scale=SCALE, num_splits=n, variant=variant)
        Of, Lf = fa.flash_attention_mla_sparse_decode_forward(Q4, KV, idx4, lens_of(LENS), DEV, scale=SCALE, num_splits=n, variant=variant)
        assert same_bits(O.view(B, N_q, H, 512), Of.permute(0, 2, 1, 3)), (dtype, variant, N_q, n)
        assert same_bits(L.view(H, B, N_q), Lf.permute(1, 0, 2)), (dtype, variant, N_q, n)


def launch(Q, K, V, idx, cu, max_q, lens, variant, n, O=None, L=None, ws=None, kd=None, vd=None, block_table=None):
    """fa2_fwd_kvcache_mla_sparse_varlen itself (outputs and workspace given or allocated here) -> (O, L)"""
    total, H, _ = Q.shape
    d_v = V.shape[3]
    O = torch.empty(total, H, d_v, dtype=Q.dtype, device=DEV) if O is None else O
    L = torch.empty(H, total, dtype=Q.dtype, device=DEV) if L is None else L
    if ws is None and n > 1:
        ws = torch.empty(_lib.kvcache_varlen_workspace_bytes(total, H, d_v, n) // 4, dtype=torch.float32, device=DEV)
    _lib.fa2_fwd_kvcache_mla_sparse_varlen(Q, K, V, O, L, idx, cu, max_q, lens, convert_triton_dtype(Q.dtype), convert_triton_dtype(K.dtype),
                                           k_descale=kd, v_descale=vd, block_table=block_table, scale=SCALE, num_splits=n, workspace=ws,
                                           variant=MLA[variant])
    return O, L


def named_rows(idx, H_kv, nq=NQ, lens=LENS):
    """bool (B, H_kv, S_K): the cache rows some list of the sequence names as a key"""
    named = torch.zeros(len(nq), H_kv, S_K, dtype=torch.bool, device=DEV)
    st = starts(nq)
    for b in range(len(nq)):
        for hk in range(H_kv):
            j = idx[st[b]:st[b + 1], hk].flatten().long()
            named[b, hk, j[(j >= 0) & (j < lens[b])]] = True
    return named


@pytest.mark.parametrize("dtype,variant", [(BF16, "mla16"), (F16, "mla16"), (BF16, "generic"), (F32, "generic")], ids=ids)
def test_only_listed_rows_are_read_poison_and_canaries(dtype, variant):
    """every cache row no list names, every row behind N_k(b) and the workspace filled with NaN, +inf or -inf: no bit of O or L moves;
    canary arenas round O, L and the partials stay intact"""
    H, H_kv, topk = 32, 2, 130
    Q, KV, _ = inputs(dtype, H, H_kv)
    idx = lists(H_kv, topk, 42)
    named = named_rows(idx, H_kv)
    assert named.any() and not named[2].any() and (~named).sum() > B * S_K // 2
    cu, lt = cu_of(CU), lens_of(LENS)
    for n in (1, 3, 16):
        words = max(_lib.kvcache_varlen_workspace_bytes(TOTAL, H, 512, n) // 4, 1)
        results = []
        for poison in (None, math.nan, math.inf, -math.inf):
            cache = KV.clone()
            if poison is not None:
                cache[~named] = poison
            O, O_all, O_sl = arena(TOTAL * H * 512, dtype, 77.0)
            L, L_all, L_sl = arena(H * TOTAL, dtype, 77.0)
            ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
            ws.fill_(0.0 if poison is None else math.nan)
            O3, L2 = launch(Q, cache, cache[..., :512], idx, cu, MAX_Q, lt, variant, n, O.view(TOTAL, H, 512), L.view(H, TOTAL), ws)
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
            if n > 1:
                assert not torch.isnan(ws).any()  # every (split, row) partial was written: every row has an owner
            results.append((O3.clone(), L2.clone()))
        assert not torch.isnan(results[0][0].float()).any()
        for O3, L2 in results[1:]:
            assert same_bits(O3, results[0][0]) and same_bits(L2, results[0][1]), (variant, n)


@pytest.mark.parametrize("variant", ["mla16", "generic"])
def test_rows_no_sequence_owns_are_not_written(variant):
    """max_seqlen_q = 2 under counts [3, 0, 1, 5, 2], and offsets that end before total_q: the surplus rows keep what O and L held, in
    the one-split and the split path; the owned rows are the full call's, bit for bit"""
    H, topk = 16, 64
    Q, KV, _ = inputs(BF16, H, 1)
    idx = lists(1, topk, 43)
    lt = lens_of(LENS)
    for n in (1, 3):
        O_full, L_full = launch(Q, KV, KV[..., :512], idx, cu_of(CU), MAX_Q, lt, variant, n)
        for cu, max_q, owned in ((CU, 2, [0, 1, 3, 4, 5, 9, 10]), ([0, 3, 3, 4, 6, 6], MAX_Q, [0, 1, 2, 3, 4, 5])):
            O = torch.full((TOTAL, H, 512), 77.0, dtype=BF16, device=DEV)
            L = torch.full((H, TOTAL), 77.0, dtype=BF16, device=DEV)
            launch(Q, KV, KV[..., :512], idx, cu_of(cu), max_q, lt, variant, n, O, L)
            rest = [t for t in range(TOTAL) if t not in owned]
            assert (O[rest] == 77.0).all() and (L[:, rest] == 77.0).all(), (variant, n, cu)
            assert same_bits(O[owned], O_full[owned]) and same_bits(L[:, owned], L_full[:, owned]), (variant, n, cu)


@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("cu", [[0, 3, 2, 4, 9, 11], [0, 3, 3, 4, 9, 40], [5, -7, 3, 2 ** 31 - 1, -2 ** 31, 1], [11] * 6, [0] * 6], ids=ids)
def test_malformed_offsets_stay_inside_the_tensors(cu, variant):
    """a decreasing entry, an entry past total_q, wild entries: wrong results are allowed, the canary arenas round O, L and the
    partials stay intact (and so does a paged pool's table walk: the sequence found for a row lies in [0, B))"""
    H, H_kv, topk = 32, 2, 130
    Q, KV, _ = inputs(BF16, H, H_kv)
    idx = lists(H_kv, topk, 44)
    pool, table = paged(KV, 16, 45)
    for n in (1, 3):
        for K, tb in ((KV, None), (pool, table)):
            words = max(_lib.kvcache_varlen_workspace_bytes(TOTAL, H, 512, n) // 4, 1)
            O, O_all, O_sl = arena(TOTAL * H * 512, BF16, 77.0)
            L, L_all, L_sl = arena(H * TOTAL, BF16, 77.0)
            ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
            launch(Q, K, K[..., :512], idx, cu_of(cu), MAX_Q, lens_of(LENS), variant, n, O.view(TOTAL, H, 512), L.view(H, TOTAL), ws, block_table=tb)
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)


@pytest.mark.parametrize("H,H_kv", HEADS)
@pytest.mark.parametrize("dtype,variant", [(F16, "mla16"), (BF16, "mla16"), (F16, "generic"), (BF16, "generic"), (F32, "generic")], ids=ids)
def test_forward_against_fp64_truth(dtype, variant, H, H_kv):
    """O and L against sparse_reference per sequence under check_forward's bars for the dtype"""
    Q, KV, _ = inputs(dtype, H, H_kv)
    st = starts(NQ)
    for topk, n in ((64, 1), (130, 3), (130, 0)):
        idx = lists(H_kv, topk, 7 * H + topk)
        O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx, cu_of(CU), MAX_Q, lens_of(LENS), DEV, scale=SCALE, num_splits=n,
                                                                   variant=variant)
        for b, cnt in enumerate(NQ):
            if cnt == 0:
                continue
            s, e = st[b], st[b + 1]
            O_ref, L_ref = sparse_reference(Q[s:e].transpose(0, 1)[None], KV[b:b + 1].double(), KV[b:b + 1, ..., :512].double(),
                                            idx[s:e].transpose(0, 1)[None], LENS[b:b + 1], SCALE)
            check_forward(O[s:e].transpose(0, 1)[None], L[:, s:e][None], O_ref, L_ref, dtype, (dtype, variant, H, H_kv, topk, n, b))


def test_two_dimensional_indices_expand_over_the_kv_heads():
    """(total_q, topk) is the same list for every KV head, passed without a copy (head stride 0)"""
    Q, KV, _ = inputs(BF16, 32, 2)
    idx = lists(1, 130, 46)
    for variant in ("mla16", "generic"):
        O2, L2 = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx[:, 0], cu_of(CU), MAX_Q, lens_of(LENS), DEV, scale=SCALE,
                                                                     variant=variant, num_splits=3)
        O3, L3 = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx.expand(-1, 2, -1).contiguous(), cu_of(CU), MAX_Q, lens_of(LENS),
                                                                     DEV, scale=SCALE, variant=variant, num_splits=3)
        assert same_bits(O2, O3) and same_bits(L2, L3), variant
