"""The MLA indexer on the GPU (flash_attention_mla_indexer_topk, mla_indexer_logits): exact arithmetic against the fp64 restatement
bit for bit, random data under the derived rounding bar, paged against contiguous bit for bit, only candidates read, and the lists
end to end through flash_attention_mla_sparse_decode_forward.

Random data, measured on an MI355X against the fp64 restatement of the stored operands (largest |error| / derived bar over every
case below): VALU form 0.006, matrix form 0.002 -- both forms meet the bar as derived, so both keep it."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from mla_indexer_restatement import candidate_mask, logits_bar, logits_f64, paged, topk_lists
from test_decode_gpu import arena, canaries_intact, check_forward, lens_of
from test_decode_mla_gpu import make
from test_decode_mla_sparse_gpu import sparse_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
S_K, D_I = 2560, 128
LENS = [0, 1, 63, 64, 65, 1000, 2049, S_K]
B = len(LENS)
# (H_I, N_q, causal, topk): every H_I and N_q of the issue -- 70 positions cross the matrix form's query block of 8 (and leave a last
# block of 6) --, both causal settings, every topk of the selection test
CONFIGS = [(64, 1, True, 2048), (64, 2, False, 65), (16, 3, True, 64), (40, 70, True, 63), (64, 70, False, 2048), (40, 2, True, 1),
           (16, 1, False, 2048), (40, 3, False, 64)]
# (q dtype, cache dtype or None = q's, variant)
FORMS = [(dt, c, v) for dt in (F16, BF16) for c in (None, E4, E5) for v in ("auto", "idx16", "generic")] + [(F32, None, "generic")]
ids = lambda x: str(x).replace("torch.", "")


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def exact_case(cfg):
    """integers in [-2, 2] for q and k, multiples of 1/8 in [-2, 2] for w, powers of two in [1/4, 4] for k_scale: every product and
    partial sum is a multiple of 1/32 below 2^24, exact in fp32 in any order.  fp32 masters, the fp64 truth and its lists."""
    H, N_q, causal, topk = cfg
    g = torch.Generator().manual_seed(1000 * H + N_q)
    q = torch.randint(-2, 3, (B, H, N_q, D_I), generator=g).float().to(DEV)
    k = torch.randint(-2, 3, (B, S_K, D_I), generator=g).float().to(DEV)
    w = (torch.randint(-16, 17, (B, H, N_q), generator=g).float() / 8).to(DEV)
    ks = (2.0 ** torch.randint(-2, 3, (B, S_K), generator=g).float()).to(DEV)
    truth = logits_f64(q, w, k, ks)
    assert truth.abs().max() < 2 ** 24 / 32 and torch.equal(truth * 32, (truth * 32).round())
    return q, w, k, ks, truth, topk_lists(truth, LENS, topk, causal)


def check_against(logits, indices, truth, lists, mask, what):
    got = torch.where(mask, logits[..., :S_K], torch.zeros((), device=DEV))
    want = torch.where(mask, truth, torch.zeros((), dtype=F64, device=DEV))
    assert torch.equal(got.double(), want), (what, (got.double() != want).nonzero()[:5].tolist())
    assert torch.equal(indices.cpu(), lists), (what, (indices.cpu() != lists).nonzero()[:5].tolist())


@pytest.mark.parametrize("cfg", CONFIGS, ids=ids)
@pytest.mark.parametrize("dtype,cache,variant", FORMS, ids=ids)
def test_exact_arithmetic_bit_for_bit(dtype, cache, variant, cfg):
    H, N_q, causal, topk = cfg
    q, w, k, ks, truth, lists = exact_case(cfg)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    assert lists.min() == -1 and (lists[-1] >= 0).all()  # a list that is padded, and a full sequence's
    indices, logits = fa.flash_attention_mla_indexer_topk(q.to(dtype), w, k.to(cache or dtype), lens_of(LENS), DEV, topk=topk, causal=causal,
                                                          k_scale=ks, variant=variant, return_logits=True)
    assert indices.shape == (B, N_q, topk) and indices.dtype == torch.int32 and logits.shape == (B, N_q, S_K) and logits.dtype == F32
    check_against(logits, indices, truth, lists, mask, (dtype, cache, variant, cfg))
    # the scores alone are the same kernel
    alone = fa.mla_indexer_logits(q.to(dtype), w, k.to(cache or dtype), lens_of(LENS), DEV, causal=causal, k_scale=ks, variant=variant)
    assert same_bits(torch.where(mask, alone, torch.zeros((), device=DEV)), torch.where(mask, logits, torch.zeros((), device=DEV)))


@pytest.mark.parametrize("variant", ["idx16", "generic"])
def test_exact_without_k_scale_and_strided_operands(variant):
    """k_scale is optional over a 16-bit cache (None = 1); q_idx, weights and k_idx as non-contiguous views"""
    cfg = (40, 3, True, 64)
    H, N_q, causal, topk = cfg
    q, w, k, _, _, _ = exact_case(cfg)
    truth = logits_f64(q, w, k)
    lists = topk_lists(truth, LENS, topk, causal)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    qv = q.to(BF16).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)  # (B, N_q, H, d) in memory: MLA's projection layout
    wv = w.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    kv = torch.zeros(B, S_K, 2 * D_I, dtype=BF16, device=DEV)[..., :D_I]
    kv.copy_(k)
    assert not qv.is_contiguous() and not wv.is_contiguous() and not kv.is_contiguous()
    indices, logits = fa.flash_attention_mla_indexer_topk(qv, wv, kv, lens_of(LENS), DEV, topk=topk, causal=causal, variant=variant,
                                                          return_logits=True)
    check_against(logits, indices, truth, lists, mask, variant)


@pytest.mark.parametrize("page", [1, 16, 48, 64])
@pytest.mark.parametrize("cache", [None, E4], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "idx16", "generic"])
def test_paged_equals_contiguous_bit_for_bit(variant, cache, page):
    """a shuffled table, NaN decoy rows (and scales) in the spare pages and behind the last row, one wild table entry"""
    cfg = (40, 3, True, 64)
    H, N_q, causal, topk = cfg
    q, w, k, ks, truth, lists = exact_case(cfg)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    pool, spool, table = paged(k.to(cache or BF16), ks, page, seed=page, lens=LENS)
    assert table.max() == 2 ** 30 and torch.isnan(pool.float()).any()
    indices, logits = fa.flash_attention_mla_indexer_topk(q.to(BF16), w, pool, lens_of(LENS), DEV, topk=topk, causal=causal, k_scale=spool,
                                                          block_table=table, variant=variant, return_logits=True)
    assert logits.shape == (B, N_q, table.shape[1] * page)
    check_against(logits, indices, truth, lists, mask, (variant, cache, page))
    flat, flat_logits = fa.flash_attention_mla_indexer_topk(q.to(BF16), w, k.to(cache or BF16), lens_of(LENS), DEV, topk=topk, causal=causal,
                                                            k_scale=ks, variant=variant, return_logits=True)
    assert torch.equal(indices, flat)
    assert same_bits(torch.where(mask, logits[..., :S_K], torch.zeros((), device=DEV)), torch.where(mask, flat_logits, torch.zeros((), device=DEV)))


@functools.lru_cache(maxsize=None)
def random_case(cfg, dtype, cache):
    """normal q, k, w; the fp64 restatement and the derived bar of the STORED operands (16-bit, or the dequantised fp8 rows)"""
    H, N_q, causal, _ = cfg
    g = torch.Generator().manual_seed(77 * H + N_q)
    q = torch.randn(B, H, N_q, D_I, generator=g).to(dtype).to(DEV)
    k = torch.randn(B, S_K, D_I, generator=g).to(DEV)
    w = (torch.randn(B, H, N_q, generator=g) * H ** -0.5).to(DEV)
    if cache is None:
        k, ks = k.to(dtype), None
    else:
        k, ks = fa.quantize_index_keys(k, cache)
    return q, w, k, ks, logits_f64(q, w, k.float(), ks), logits_bar(q, w, k.float(), ks)


RANDOM_FORMS = [(dt, c, v) for dt in (F16, BF16) for c in (None, E4) for v in ("idx16", "generic")] + [(BF16, E5, "auto"), (F32, None, "generic")]


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2], CONFIGS[3], CONFIGS[4]], ids=ids)
@pytest.mark.parametrize("dtype,cache,variant", RANDOM_FORMS, ids=ids)
def test_random_data_under_the_derived_bar(dtype, cache, variant, cfg):
    """|err[j]| <= (d_I + H_I + 2) 2^-24 k_scale[j] sum_h |w[h]| sum_c |q[h, c] k[j, c]|: fp32 accumulation of d_I + H_I + 2 terms in any
    order, per element.  The fused call's lists are the selection of its own logits, exactly."""
    H, N_q, causal, topk = cfg
    q, w, k, ks, truth, bar = random_case(cfg, dtype, cache)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    indices, logits = fa.flash_attention_mla_indexer_topk(q, w, k, lens_of(LENS), DEV, topk=topk, causal=causal, k_scale=ks, variant=variant,
                                                          return_logits=True)
    err = (logits.double() - truth).abs()
    ratio = torch.where(mask & (bar > 0), err / bar.clamp(min=1e-300), torch.zeros((), dtype=F64, device=DEV)).max().item()
    print(f"{ids(dtype)} {ids(cache)} {variant} {cfg}: largest |error| / bar = {ratio:.3f}")
    assert not torch.isnan(logits[mask]).any()
    assert (err[mask] <= bar[mask]).all(), ratio
    assert torch.equal(indices, fa.topk_indices(logits, lens_of(LENS), topk, causal=causal))
    assert torch.equal(indices.cpu(), topk_lists(logits, LENS, topk, causal))


@pytest.mark.parametrize("variant", ["idx16", "generic"])
@pytest.mark.parametrize("cache", [None, E4], ids=ids)
@pytest.mark.parametrize("page", [0, 48])
def test_only_candidates_are_read_and_written(page, cache, variant):
    """cache rows at and behind N_k(b), their scales, the spare pages and the logits buffer hold NaN / inf: the lists and the
    candidates' logits do not move by a bit, nothing else of the logits buffer is written, and the canaries stay intact"""
    cfg = (40, 3, True, 64)
    H, N_q, causal, topk = cfg
    q, w, k, ks, _ = random_case(cfg, BF16, cache)[:5]
    if ks is None:
        ks = torch.ones(B, S_K, device=DEV)
    lens = lens_of(LENS)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    behind = torch.arange(S_K, device=DEV)[None, :] >= lens[:, None]
    enum, kenum = convert_triton_dtype(BF16), convert_triton_dtype(k.dtype)
    results = []
    for poison in (False, True):
        kk, kss = k.clone(), ks.clone()
        if poison:  # (through fp32 and back: the stored values are the format's, so the bytes of the other rows do not change)
            kk = torch.where(behind[..., None], torch.full((), float("nan"), device=DEV), k.float()).to(k.dtype)
            kss = torch.where(behind, torch.full((), float("nan"), device=DEV), ks)
        table = None
        if page:
            kk, kss, table = paged(kk, kss, page, seed=3, fill=float("nan") if poison else 0.0, lens=LENS)
        cap = kk.shape[1] * (table.shape[1] if page else 1)
        junk = float("inf") if poison else -5.0
        logits, lg_all, lg_sl = arena(B * N_q * cap, F32, junk)
        indices, ix_all, ix_sl = arena(B * N_q * topk, torch.int32, -77)
        logits, indices = logits.view(B, N_q, cap), indices.view(B, N_q, topk)
        _lib.fa2_mla_indexer_topk(q, w, kk, kss, logits, indices, lens, enum, kenum, block_table=table, causal=causal,
                                  variant=_lib.INDEXER_VARIANTS[variant])
        torch.cuda.synchronize()
        assert canaries_intact(lg_all, lg_sl, junk) and canaries_intact(ix_all, ix_sl, -77)
        full = torch.zeros(B, N_q, cap, dtype=torch.bool, device=DEV)
        full[..., :S_K] = mask
        assert (logits[~full] == junk).all()  # no entry that is no candidate is written
        assert not torch.isnan(logits[full]).any() and not torch.isinf(logits[full]).any()
        results.append((logits[full].clone(), indices.clone()))
    assert same_bits(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_end_to_end_identity_lists_equal_the_dense_call_bit_for_bit(dtype):
    """N_q = 1 over sequences of 640 keys with topk = 640: the indexer's lists are the identity, and the sparse call on them is the
    dense latent call bit for bit (what test_identity_list_equals_the_dense_call_bit_for_bit pins for a hand-made identity)"""
    Bq, H, N_q, N_k, scale = 3, 64, 1, 640, 576 ** -0.5
    Q, KV = make(Bq, H, N_q, N_k, dtype, 31)
    g = torch.Generator().manual_seed(5)
    q_idx = torch.randn(Bq, 64, N_q, D_I, generator=g).to(dtype).to(DEV)
    k_idx = torch.randn(Bq, N_k, D_I, generator=g).to(dtype).to(DEV)
    w = torch.randn(Bq, 64, N_q, generator=g).to(DEV)
    idx = fa.flash_attention_mla_indexer_topk(q_idx, w, k_idx, None, DEV, topk=N_k)
    assert torch.equal(idx, torch.arange(N_k, dtype=torch.int32, device=DEV).expand(Bq, N_q, N_k))
    O, L = fa.flash_attention_mla_sparse_decode_forward(Q, KV, idx, None, DEV, scale=scale, variant="mla16")
    Od, Ld = fa.flash_attention_mla_decode_forward(Q, KV, None, DEV, scale=scale, variant="mla16")
    assert not torch.isnan(O.float()).any()
    assert torch.equal(O.view(torch.int16), Od.view(torch.int16)) and torch.equal(L.view(torch.int16), Ld.view(torch.int16))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_end_to_end_short_lists_meet_the_sparse_truth(dtype):
    """topk = 64 < N_k, N_q = 2: the sparse call on the indexer's lists against the fp64 truth on the same lists, check_forward's bars"""
    Bq, H, N_q, N_k, topk, scale = 3, 64, 2, 640, 64, 576 ** -0.5
    lens = [640, 64, 333]
    Q, KV = make(Bq, H, N_q, N_k, dtype, 41)
    g = torch.Generator().manual_seed(6)
    q_idx = torch.randn(Bq, 64, N_q, D_I, generator=g).to(dtype).to(DEV)
    k_idx = torch.randn(Bq, N_k, D_I, generator=g).to(dtype).to(DEV)
    w = torch.randn(Bq, 64, N_q, generator=g).to(DEV)
    idx, logits = fa.flash_attention_mla_indexer_topk(q_idx, w, k_idx, lens_of(lens), DEV, topk=topk, return_logits=True)
    assert torch.equal(idx.cpu(), topk_lists(logits, lens, topk, True))
    assert idx[1, 0, -1] == -1 and (idx[1, 1] >= 0).all()  # 64 keys: the first position has 63 candidates, the second 64
    assert not torch.equal(idx[0, 0], torch.arange(topk, dtype=torch.int32, device=DEV))  # a selection, not a prefix
    O, L = fa.flash_attention_mla_sparse_decode_forward(Q, KV, idx, lens_of(lens), DEV, scale=scale, variant="mla16")
    O_ref, L_ref = sparse_reference(Q, KV.double(), KV[..., :512].double(), idx[:, None], lens, scale)
    check_forward(O, L, O_ref, L_ref, dtype, ("indexer lists", dtype))
