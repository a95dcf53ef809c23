"""The MLA indexer with fp8 queries (the _q8 entry points) on the GPU: idx8 and the VALU form against the fp64 restatement; end to end."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from mla_indexer_restatement import candidate_mask, logits_bar, logits_f64, paged, topk_lists
from test_decode_gpu import check_forward, lens_of
from test_decode_mla_gpu import make
from test_decode_mla_sparse_gpu import sparse_reference

pytestmark, DEV = pytest.mark.gpu, torch.device("cuda:0")
F64, E4, E5 = torch.float64, torch.float8_e4m3fn, torch.float8_e5m2
S_K, D_I = 384, 128
LENS, B = [0, 1, 63, 64, 65, 200, 321, S_K], 8
CONFIGS = [  # (H_I, N_q, causal, topk): 17 and 35 positions cross the matrix form's query block of 16
    (64, 1, True, 64), (64, 17, False, 65), (16, 2, False, 63), (16, 35, True, 64), (40, 3, True, 1), (40, 35, False, 400)]
ids = lambda x: str(x).replace("torch.", "")
zero = lambda t: torch.zeros((), dtype=t.dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def exact_case(cfg):
    H, N_q, causal, topk = cfg  # integers in [-2, 2] for q and k, eighths for w, powers of two for k_scale: exact in fp32 in any order
    g = torch.Generator().manual_seed(1000 * H + N_q)
    q = torch.randint(-2, 3, (B, H, N_q, D_I), generator=g).float().to(DEV)
    k = torch.randint(-2, 3, (B, S_K, D_I), generator=g).float().to(DEV)
    w = (torch.randint(-16, 17, (B, H, N_q), generator=g).float() / 8).to(DEV)
    ks = (2.0 ** torch.randint(-2, 3, (B, S_K), generator=g).float()).to(DEV)
    truth = logits_f64(q, w, k, ks)
    assert truth.abs().max() < 2 ** 24 / 32 and (w < 0).any()
    return q, w, k, ks, truth, topk_lists(truth, LENS, topk, causal)


@pytest.mark.parametrize("cfg", CONFIGS, ids=ids)
@pytest.mark.parametrize("qt,kt", [(E4, E4), (E4, E5), (E5, E4), (E5, E5)], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "idx8", "generic"])
def test_exact_arithmetic_bit_for_bit(variant, qt, kt, cfg):
    H, N_q, causal, topk = cfg
    q, w, k, ks, truth, lists = exact_case(cfg)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    indices, logits = fa.flash_attention_mla_indexer_topk(q.to(qt), w, k.to(kt), lens_of(LENS), DEV, topk=topk, causal=causal, k_scale=ks,
                                                          variant=variant, return_logits=True)
    assert torch.equal(torch.where(mask, logits, zero(logits)).double(), torch.where(mask, truth, zero(truth)))
    assert torch.equal(indices.cpu(), lists)


@pytest.mark.parametrize("page", [1, 16, 48, 64])
@pytest.mark.parametrize("variant,qt,kt", [("idx8", E4, E4), ("idx8", E5, E4), ("auto", E4, E5), ("generic", E4, E4)], ids=ids)
def test_paged_equals_contiguous_and_only_candidates_are_touched(variant, qt, kt, page):
    cfg = (40, 35, True, 64)  # a shuffled table, one wild entry, fp8 NaN bytes (0x7f) behind cache_seqlens[b] and in spare pages, a canary
    H, N_q, causal, topk = cfg
    q, w, k, ks, truth, _ = exact_case(cfg)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    k8 = k.to(kt)
    for b, n in enumerate(LENS):
        k8.view(torch.uint8)[b, n:] = 0x7f
    pool, spool, table = paged(k8, ks, page, seed=page, lens=LENS)
    assert table.max() == 2 ** 30 and torch.isnan(pool.float()).any() and torch.isnan(k8[:-1].float()).any()
    both = []
    for cache, scale, tb in ((k8, ks, None), (pool, spool, table)):
        logits = torch.full((B, N_q, (tb.shape[1] * page) if tb is not None else S_K), -7.25, device=DEV)
        _lib.fa2_mla_indexer_logits(q.to(qt), w, cache, scale, logits, lens_of(LENS), convert_triton_dtype(qt), convert_triton_dtype(kt),
                                    block_table=tb, causal=causal, variant=_lib.INDEXER_Q8_VARIANTS[variant])
        assert (logits[..., :S_K][~mask] == -7.25).all() and (logits[..., S_K:] == -7.25).all()
        assert torch.equal(logits[..., :S_K][mask].double(), truth[mask])
        both.append(logits[..., :S_K])
    assert torch.equal(both[0].view(torch.int32), both[1].view(torch.int32))


@functools.lru_cache(maxsize=None)
def random_case(H, N_q, causal):
    """normal q, k, w; q and k quantised to e4m3, the queries' scale folded into w; the fp64 restatement and bar of the STORED operands"""
    g = torch.Generator().manual_seed(77 * H + N_q)
    q8, qs = fa.quantize_index_keys(torch.randn(B, H, N_q, D_I, generator=g).to(DEV), E4)
    k8, ks = fa.quantize_index_keys(torch.randn(B, S_K, D_I, generator=g).to(DEV), E4)
    w = (torch.randn(B, H, N_q, generator=g) * H ** -0.5).to(DEV) * qs
    return q8, w, k8, ks, logits_f64(q8.float(), w, k8.float(), ks), logits_bar(q8.float(), w, k8.float(), ks)


@pytest.mark.parametrize("H,N_q,causal", [(64, 35, True), (40, 17, False), (16, 2, True)])
@pytest.mark.parametrize("variant", ["idx8", "generic"])
def test_random_data_under_the_derived_bar(variant, H, N_q, causal):
    """|err[j]| <= (d_I + H_I + 2) 2^-24 k_scale[j] sum_h |w[h]| sum_c |q[h, c] k[j, c]|, both forms.  Largest ratios seen ("MLA
    indexer: fp8 queries"): idx8 0.27 (the instruction does not sum like an fp32 chain, yet keeps the bar), generic 0.002."""
    q8, w, k8, ks, truth, bar = random_case(H, N_q, causal)
    mask = candidate_mask(LENS, B, N_q, S_K, causal, DEV)
    indices, logits = fa.flash_attention_mla_indexer_topk(q8, w, k8, lens_of(LENS), DEV, topk=64, causal=causal, k_scale=ks, variant=variant,
                                                          return_logits=True)
    ratio = torch.where(mask & (bar > 0), (logits.double() - truth).abs() / bar.clamp(min=1e-300), zero(truth)).max().item()
    print(f"q8 indexer {variant} H_I={H} N_q={N_q} causal={causal}: largest error / bar = {ratio:.4f}")
    assert ratio <= 1.0, ratio
    assert torch.equal(indices.cpu(), topk_lists(logits, LENS, 64, causal))


@pytest.mark.parametrize("variant", ["idx8", "generic"])
def test_packed_rows_equal_the_fixed_call_bit_for_bit(variant):
    H, causal, lens, n_q = 40, True, [64, 321, 1, S_K, 200], [0, 19, 1, 1, 3]  # an empty sequence, a chunk of 19 rows, one-token ones
    q8, w, k8, ks, _, _ = random_case(H, 35, True)
    cu = torch.tensor([0, 0, 19, 20, 21, 24], dtype=torch.int32, device=DEV)
    qp = torch.cat([q8[b, :, :n].transpose(0, 1) for b, n in enumerate(n_q)]).contiguous()  # (total_q, H, d)
    wp = torch.cat([w[b, :, :n].T for b, n in enumerate(n_q)]).contiguous()
    indices, logits = fa.flash_attention_mla_indexer_topk_varlen(qp, wp, k8[:5], cu, 19, lens_of(lens), DEV, topk=64, causal=causal, k_scale=ks[:5],
                                                                 variant=variant, return_logits=True)
    assert torch.equal(indices, fa.topk_indices_varlen(logits, cu, 19, lens_of(lens), 64, causal=causal))
    for b, n in enumerate(n_q):
        if n:
            alone = fa.mla_indexer_logits(q8[b:b + 1, :, :n], w[b:b + 1, :, :n], k8[b:b + 1], lens_of(lens[b:b + 1]), DEV, causal=causal,
                                          k_scale=ks[b:b + 1], variant=variant)
            mask = candidate_mask(lens[b:b + 1], 1, n, S_K, causal, DEV)[0]
            rows = logits[int(cu[b]):int(cu[b]) + n]
            assert torch.equal(torch.where(mask, rows, zero(rows)).view(torch.int32), torch.where(mask, alone[0], zero(rows)).view(torch.int32)), b


def test_end_to_end_short_lists_meet_the_sparse_truth():
    Bq, N_q, N_k, topk, scale, lens = 3, 2, 640, 64, 576 ** -0.5, [640, 64, 333]
    Q, KV = make(Bq, 64, N_q, N_k, torch.bfloat16, 41)
    g = torch.Generator().manual_seed(6)
    q8, qs = fa.quantize_index_keys(torch.randn(Bq, 64, N_q, D_I, generator=g).to(DEV), E4)
    k8, ks = fa.quantize_index_keys(torch.randn(Bq, N_k, D_I, generator=g).to(DEV), E4)
    w = torch.randn(Bq, 64, N_q, generator=g).to(DEV) * qs
    idx, logits = fa.flash_attention_mla_indexer_topk(q8, w, k8, lens_of(lens), DEV, topk=topk, k_scale=ks, variant="idx8", return_logits=True)
    assert torch.equal(idx.cpu(), topk_lists(logits, lens, topk, True))
    assert idx[1, 0, -1] == -1 and not torch.equal(idx[0, 0], torch.arange(topk, dtype=torch.int32, device=DEV))
    O, L = fa.flash_attention_mla_sparse_decode_forward(Q, KV, idx, lens_of(lens), DEV, scale=scale, variant="mla16")
    O_ref, L_ref = sparse_reference(Q, KV.double(), KV[..., :512].double(), idx[:, None], lens, scale)
    check_forward(O, L, O_ref, L_ref, torch.bfloat16, "idx8 lists")
