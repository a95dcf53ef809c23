"""The MLA indexer over packed queries on the GPU (flash_attention_mla_indexer_topk_varlen, mla_indexer_logits_varlen,
topk_indices_varlen).  Exact-arithmetic data, as tests/test_mla_indexer_gpu.py makes it: the logits of every sequence equal the fp64
restatement (tests/mla_indexer_restatement.py) on that sequence alone bit for bit, and equal the fixed call on that sequence's slice bit
for bit; the lists equal exactly.  Paged against contiguous bit for bit, a logits buffer pre-filled with a NaN pattern whose
non-candidates keep their bits, the selection alone on the fixed selection test's seven kinds of logits, and the lists end to end
through flash_attention_mla_sparse_varlen_decode_forward against the per-sequence fixed pipeline and the dense packed call.  The edge
batch of tests/mla_sparse_varlen_probe.py (a leading empty sequence, two in a row, a trailing one, B = 11) through the selection and
the fused call, for the owner search they share with the packed sparse kernels."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_sparse_varlen_probe as EV
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from mla_indexer_restatement import candidate_mask, logits_f64, paged, topk_lists
from test_decode_gpu import arena, canaries_intact, lens_of
from test_mla_indexer_topk_gpu import KINDS, make_logits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
# the ragged batch: 8, 9 and 19 positions meet and cross the matrix form's query block of 8; a sequence without a token; the last
# sequence is shorter than its query count (positions without a candidate)
NQ = [3, 0, 1, 19, 8, 9, 5]
LENS = [70, 10, 1, 300, 64, 2100, 2]
B, S_K, D_I, MAX_Q, TOTAL = len(NQ), 2100, 128, max(NQ), sum(NQ)
ST = [sum(NQ[:b]) for b in range(B + 1)]
HEADS = (64, 16, 40)
TOPKS = (64, 2048)  # the selection runs; the identity prefix on every sequence but the one of 2,100 keys
# (q dtype, cache dtype or None = q's, variant)
FORMS = [(dt, c, v) for dt in (F16, BF16) for c in (None, E4, E5) for v in ("auto", "idx16", "generic")] + [(F32, None, "generic")]
ids = lambda x: str(x).replace("torch.", "")


def cu_of(values=ST):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def seq_view(q, w, b):
    """the fixed call's (1, H, n, d) and (1, H, n) views of sequence b's packed rows"""
    s, e = ST[b], ST[b + 1]
    return q[s:e].transpose(0, 1)[None], w[s:e].transpose(0, 1)[None]


@functools.lru_cache(maxsize=None)
def exact_case(H):
    """integers in [-2, 2] for q and k, multiples of 1/8 in [-2, 2] for w, powers of two in [1/4, 4] for k_scale: every product and
    partial sum is a multiple of 1/32 below 2^24, exact in fp32 in any order.  fp32 masters and the packed fp64 truth, made of the
    restatement on each sequence alone."""
    g = torch.Generator().manual_seed(1000 * H + 7)
    q = torch.randint(-2, 3, (TOTAL, H, D_I), generator=g).float().to(DEV)
    k = torch.randint(-2, 3, (B, S_K, D_I), generator=g).float().to(DEV)
    w = (torch.randint(-16, 17, (TOTAL, H), generator=g).float() / 8).to(DEV)
    ks = (2.0 ** torch.randint(-2, 3, (B, S_K), generator=g).float()).to(DEV)
    truth = torch.zeros(TOTAL, S_K, dtype=F64, device=DEV)
    for b in range(B):
        if NQ[b]:
            qb, wb = seq_view(q, w, b)
            truth[ST[b]:ST[b + 1]] = logits_f64(qb, wb, k[b:b + 1], ks[b:b + 1])[0]
    assert truth.abs().max() < 2 ** 24 / 32 and torch.equal(truth * 32, (truth * 32).round())
    return q, w, k, ks, truth


@functools.lru_cache(maxsize=None)
def packed_mask(causal):
    """bool (total_q, S_K): j < n of the row, the fixed call's count with n_q(b) in N_q's place"""
    mask = torch.zeros(TOTAL, S_K, dtype=torch.bool, device=DEV)
    for b in range(B):
        if NQ[b]:
            mask[ST[b]:ST[b + 1]] = candidate_mask(LENS[b:b + 1], 1, NQ[b], S_K, causal, DEV)[0]
    return mask


def packed_lists(logits, topk, causal):
    """the restatement's lists of packed logits (total_q, S_K), sequence by sequence -> int32 (total_q, topk) on the CPU"""
    out = torch.empty(TOTAL, topk, dtype=torch.int32)
    for b in range(B):
        if NQ[b]:
            out[ST[b]:ST[b + 1]] = topk_lists(logits[None, ST[b]:ST[b + 1]], LENS[b:b + 1], topk, causal)[0]
    return out


@functools.lru_cache(maxsize=None)
def exact_lists(H, topk, causal):
    return packed_lists(exact_case(H)[4], topk, causal)


def masked(logits, mask):
    return torch.where(mask, logits[..., :S_K], torch.zeros((), dtype=logits.dtype, device=DEV))


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("dtype,cache,variant", FORMS, ids=ids)
def test_exact_arithmetic_equals_the_restatement_and_the_fixed_call_bit_for_bit(dtype, cache, variant, H):
    q, w, k, ks, truth = exact_case(H)
    qd, kd = q.to(dtype), k.to(cache or dtype)
    lens = lens_of(LENS)
    for causal in (True, False):
        mask = packed_mask(causal)
        if causal:
            assert not mask[ST[6]:ST[6] + 3].any() and mask[ST[6] + 3, 0] and mask[ST[6] + 4, :2].all()  # 2 keys under 5 queries
        for topk in TOPKS:
            lists = exact_lists(H, topk, causal)
            what = (dtype, cache, variant, H, causal, topk)
            indices, logits = fa.flash_attention_mla_indexer_topk_varlen(qd, w, kd, cu_of(), MAX_Q, lens, DEV, topk=topk, causal=causal,
                                                                         k_scale=ks, variant=variant, return_logits=True)
            assert indices.shape == (TOTAL, topk) and indices.dtype == torch.int32 and logits.shape == (TOTAL, S_K) and logits.dtype == F32
            # the restatement: logits bit for bit (exact data: equality of the values is equality of the bits, -0.0 aside, which an fp64
            # sum of these terms does not produce either), lists exactly
            assert torch.equal(masked(logits, mask).double(), masked(truth, mask)), what
            assert torch.equal(indices.cpu(), lists), (what, (indices.cpu() != lists).nonzero()[:5].tolist())
            # the fixed call on each sequence's slice
            for b in range(B):
                if NQ[b] == 0:
                    continue
                qb, wb = seq_view(qd, w, b)
                ib, lb = fa.flash_attention_mla_indexer_topk(qb, wb, kd[b:b + 1], lens[b:b + 1], DEV, topk=topk, causal=causal,
                                                             k_scale=ks[b:b + 1], variant=variant, return_logits=True)
                mb = mask[ST[b]:ST[b + 1]]
                assert same_bits(masked(logits[ST[b]:ST[b + 1]], mb), masked(lb[0], mb)), (what, b)
                assert torch.equal(indices[ST[b]:ST[b + 1]], ib[0]), (what, b)
        # the scores alone are the same kernel
        alone = fa.mla_indexer_logits_varlen(qd, w, kd, cu_of(), MAX_Q, lens, DEV, causal=causal, k_scale=ks, variant=variant)
        assert same_bits(masked(alone, mask), masked(logits, mask)), (dtype, cache, variant, H, causal)


@pytest.mark.parametrize("page", [1, 16, 48, 64])
@pytest.mark.parametrize("cache", [None, E4], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "idx16", "generic"])
def test_paged_equals_contiguous_bit_for_bit(variant, cache, page):
    """a shuffled table, NaN decoy rows (and scales) in the spare pages and behind the last row, one wild table entry"""
    H, topk, causal = 40, 64, True
    q, w, k, ks, truth = exact_case(H)
    mask = packed_mask(causal)
    pool, spool, table = paged(k.to(cache or BF16), ks, page, seed=page, lens=LENS)
    assert table.max() == 2 ** 30 and torch.isnan(pool.float()).any()
    indices, logits = fa.flash_attention_mla_indexer_topk_varlen(q.to(BF16), w, pool, cu_of(), MAX_Q, lens_of(LENS), DEV, topk=topk, causal=causal,
                                                                 k_scale=spool, block_table=table, variant=variant, return_logits=True)
    assert logits.shape == (TOTAL, table.shape[1] * page)
    flat, flat_logits = fa.flash_attention_mla_indexer_topk_varlen(q.to(BF16), w, k.to(cache or BF16), cu_of(), MAX_Q, lens_of(LENS), DEV, topk=topk,
                                                                   causal=causal, k_scale=ks, variant=variant, return_logits=True)
    assert torch.equal(indices, flat) and torch.equal(indices.cpu(), exact_lists(H, topk, causal))
    assert same_bits(masked(logits, mask), masked(flat_logits, mask))
    assert torch.equal(masked(logits, mask).double(), masked(truth, mask))


NAN_PATTERN = 0x7fc12345


@pytest.mark.parametrize("variant", ["idx16", "generic"])
@pytest.mark.parametrize("causal", [True, False])
def test_logits_buffer_keeps_the_bits_of_every_entry_that_is_no_candidate(causal, variant):
    """the logits buffer and the lists sit in canary arenas; the buffer is pre-filled with a NaN pattern, and max_seqlen_q = 8 leaves
    rows no sequence owns (the surplus of the sequences of 19 and 9 positions): nothing of those rows, logits or list, is written"""
    H, topk = 40, 64
    q, w, k, ks, _ = exact_case(H)
    for max_q in (MAX_Q, 8):
        logits, lg_all, lg_sl = arena(TOTAL * S_K, torch.int32, NAN_PATTERN)
        indices, ix_all, ix_sl = arena(TOTAL * topk, torch.int32, -77)
        logits, indices = logits.view(TOTAL, S_K).view(F32), indices.view(TOTAL, topk)
        _lib.fa2_mla_indexer_topk_varlen(q.to(BF16), w, k.to(BF16), ks, logits, indices, cu_of(), max_q, lens_of(LENS),
                                         convert_triton_dtype(BF16), convert_triton_dtype(BF16), causal=causal,
                                         variant=_lib.INDEXER_VARIANTS[variant])
        torch.cuda.synchronize()
        assert canaries_intact(lg_all, lg_sl, NAN_PATTERN) and canaries_intact(ix_all, ix_sl, -77)
        mask = torch.zeros(TOTAL, S_K, dtype=torch.bool, device=DEV)
        owned = torch.zeros(TOTAL, dtype=torch.bool, device=DEV)
        for b in range(B):
            n = min(NQ[b], max_q)
            if n:
                mask[ST[b]:ST[b] + n] = candidate_mask(LENS[b:b + 1], 1, n, S_K, causal, DEV)[0]
                owned[ST[b]:ST[b] + n] = True
        assert (~owned).sum() == (0 if max_q == MAX_Q else 12)
        assert (logits.view(torch.int32)[~mask] == NAN_PATTERN).all()
        assert not torch.isnan(logits[mask]).any()
        assert (indices[~owned] == -77).all() and (indices[owned] != -77).all()


@functools.lru_cache(maxsize=None)
def kind_case(kind, causal):
    """packed logits (total_q, S_K) of one of the fixed selection test's seven kinds, NaN / +inf behind every row's candidates"""
    x = make_logits(kind, MAX_Q, 11 * KINDS.index(kind) + 3)  # (8, MAX_Q, 2560)
    rows = torch.cat([x[b, :NQ[b], :S_K] for b in range(B)])
    junk = torch.where(torch.arange(S_K) % 2 == 0, torch.tensor(float("nan")), torch.tensor(float("inf"))).expand(TOTAL, S_K)
    return torch.where(packed_mask(causal).cpu(), rows, junk).to(DEV)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("causal", [True, False])
def test_selection_alone_equals_the_restatement(causal, kind):
    logits = kind_case(kind, causal)
    for topk in (1, 63, 64, 65, 2048):
        want = packed_lists(logits, topk, causal)
        idx, whole, sl = arena(TOTAL * topk, torch.int32, -77)
        idx = idx.view(TOTAL, topk)
        _lib.fa2_topk_indices_varlen(logits, idx, cu_of(), MAX_Q, lens_of(LENS), causal=causal)
        torch.cuda.synchronize()
        assert canaries_intact(whole, sl, -77)
        assert torch.equal(idx.cpu(), want), (kind, causal, topk, (idx.cpu() != want).nonzero()[:5].tolist())
        # the Python surface is the same call; strided logits give the bytes of their contiguous copy
        assert torch.equal(fa.topk_indices_varlen(logits, cu_of(), MAX_Q, lens_of(LENS), topk, causal=causal).cpu(), want)
    wide = torch.full((TOTAL, 2 * S_K + 3), float("inf"), device=DEV)
    wide[:, 1:2 * S_K + 1:2] = logits
    assert torch.equal(fa.topk_indices_varlen(wide[:, 1:2 * S_K + 1:2], cu_of(), MAX_Q, lens_of(LENS), 64, causal=causal).cpu(),
                       packed_lists(logits, 64, causal))


@pytest.mark.parametrize("dtype,cache,variant", [(BF16, None, "idx16"), (F16, E4, "idx16"), (BF16, None, "generic"), (F32, None, "generic")], ids=ids)
def test_fused_lists_are_the_selection_of_its_own_logits(dtype, cache, variant):
    """random data: whatever the logits' rounding, the fused call's lists are topk_indices_varlen of the logits it wrote"""
    H, topk = 40, 64
    g = torch.Generator().manual_seed(77)
    q = torch.randn(TOTAL, H, D_I, generator=g).to(dtype).to(DEV)
    k = torch.randn(B, S_K, D_I, generator=g).to(DEV)
    w = (torch.randn(TOTAL, H, generator=g) * H ** -0.5).to(DEV)
    k, ks = (k.to(dtype), None) if cache is None else fa.quantize_index_keys(k, cache)
    for causal in (True, False):
        indices, logits = fa.flash_attention_mla_indexer_topk_varlen(q, w, k, cu_of(), MAX_Q, lens_of(LENS), DEV, topk=topk, causal=causal,
                                                                     k_scale=ks, variant=variant, return_logits=True)
        assert not torch.isnan(logits[packed_mask(causal)]).any()
        assert torch.equal(indices, fa.topk_indices_varlen(logits, cu_of(), MAX_Q, lens_of(LENS), topk, causal=causal))
        assert torch.equal(indices.cpu(), packed_lists(logits, topk, causal))


def latent(dtype, H, lens_cap, seed):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randn(TOTAL, H, 576, generator=g) * 0.5).to(dtype).to(DEV)
    KV = (torch.randn(B, 1, lens_cap, 576, generator=g) * 0.5).to(dtype).to(DEV)
    q_idx = torch.randn(TOTAL, 64, D_I, generator=g).to(dtype).to(DEV)
    k_idx = torch.randn(B, lens_cap, D_I, generator=g).to(dtype).to(DEV)
    w = torch.randn(TOTAL, 64, generator=g).to(DEV)
    return Q, KV, q_idx, k_idx, w


def bits16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_end_to_end_equals_the_per_sequence_fixed_pipeline_bit_for_bit(dtype):
    """packed indexer into the packed sparse call against fixed indexer into fixed sparse call, sequence by sequence, topk = 64"""
    H, topk, scale = 64, 64, 576 ** -0.5
    Q, KV, q_idx, k_idx, w = latent(dtype, H, S_K, 51)
    lens = lens_of(LENS)
    idx = fa.flash_attention_mla_indexer_topk_varlen(q_idx, w, k_idx, cu_of(), MAX_Q, lens, DEV, topk=topk)
    assert not torch.equal(idx[ST[5]], torch.arange(topk, dtype=torch.int32, device=DEV))  # a selection, not a prefix
    for n in (1, 3):
        O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx, cu_of(), MAX_Q, lens, DEV, scale=scale, num_splits=n)
        assert O.shape == (TOTAL, H, 512) and L.shape == (H, TOTAL) and not torch.isnan(O.float()).any()
        for b in range(B):
            if NQ[b] == 0:
                continue
            s, e = ST[b], ST[b + 1]
            qb, wb = seq_view(q_idx, w, b)
            ib = fa.flash_attention_mla_indexer_topk(qb, wb, k_idx[b:b + 1], lens[b:b + 1], DEV, topk=topk)
            assert torch.equal(ib[0], idx[s:e]), (dtype, b)
            Ob, Lb = fa.flash_attention_mla_sparse_decode_forward(Q[s:e].transpose(0, 1)[None], KV[b:b + 1], ib, lens[b:b + 1], DEV, scale=scale,
                                                                  num_splits=n)
            assert torch.equal(bits16(O[s:e]), bits16(Ob[0].transpose(0, 1))) and torch.equal(bits16(L[:, s:e]), bits16(Lb[0])), (dtype, n, b)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_end_to_end_identity_lists_equal_the_dense_packed_call_bit_for_bit(dtype):
    """every sequence holds 640 keys and topk = 640: the causal indexer's list of a query is the identity up to its position, the
    split boundaries of slots and keys coincide, and the packed sparse call on the lists is flash_attention_mla_varlen_decode_forward
    with causal=True, bit for bit at equal split counts, one split among them in both dtypes -- and the fixed dense call on each
    sequence's slice."""
    H, N_k, scale = 64, 640, 576 ** -0.5
    Q, KV, q_idx, k_idx, w = latent(dtype, H, N_k, 61)
    idx = fa.flash_attention_mla_indexer_topk_varlen(q_idx, w, k_idx, cu_of(), MAX_Q, None, DEV, topk=N_k)
    for b in range(B):
        for i in range(NQ[b]):
            p = N_k - NQ[b] + i
            want = torch.where(torch.arange(N_k) <= p, torch.arange(N_k), torch.tensor(-1)).to(torch.int32)
            assert torch.equal(idx[ST[b] + i].cpu(), want), (b, i)
    for n in (1, 3, 10):
        O, L = fa.flash_attention_mla_sparse_varlen_decode_forward(Q, KV, idx, cu_of(), MAX_Q, None, DEV, scale=scale, num_splits=n, variant="mla16")
        Od, Ld = fa.flash_attention_mla_varlen_decode_forward(Q, KV, cu_of(), MAX_Q, None, DEV, causal=True, scale=scale, num_splits=n,
                                                              variant="mla16")
        assert not torch.isnan(O.float()).any()
        assert torch.equal(bits16(O), bits16(Od)) and torch.equal(bits16(L), bits16(Ld)), (dtype, n)
        for b in range(B):
            if NQ[b] == 0:
                continue
            s, e = ST[b], ST[b + 1]
            Ob, Lb = fa.flash_attention_mla_decode_forward(Q[s:e].transpose(0, 1)[None], KV[b:b + 1], None, DEV, causal=True, scale=scale,
                                                           num_splits=n, variant="mla16")
            assert torch.equal(bits16(O[s:e]), bits16(Ob[0].transpose(0, 1))) and torch.equal(bits16(L[:, s:e]), bits16(Lb[0])), (dtype, n, b)


# ---- the edge batch of tests/mla_sparse_varlen_probe.py through the other two users of fa2_varlen_owner's search: a leading empty
# sequence, two empty sequences in a row, a trailing one, B = 11 (a search four steps deep), a sequence without a key
E_NQ, E_LENS, E_CU, E_B, E_TOTAL, E_SK, E_MAXQ = EV.N_Q, EV.N_K, EV.CU, EV.B, EV.TOTAL, EV.S_K, EV.MAX_Q


@functools.lru_cache(maxsize=None)
def edge_case(H=40):
    """exact_case's data on the edge batch: fp32 masters and the packed fp64 truth (total_q, S_k), the restatement on each sequence alone"""
    g = torch.Generator().manual_seed(1000 * H + 11)
    q = torch.randint(-2, 3, (E_TOTAL, H, D_I), generator=g).float().to(DEV)
    k = torch.randint(-2, 3, (E_B, E_SK, D_I), generator=g).float().to(DEV)
    w = (torch.randint(-16, 17, (E_TOTAL, H), generator=g).float() / 8).to(DEV)
    ks = (2.0 ** torch.randint(-2, 3, (E_B, E_SK), generator=g).float()).to(DEV)
    truth = torch.zeros(E_TOTAL, E_SK, dtype=F64, device=DEV)
    for b in range(E_B):
        if E_NQ[b]:
            s, e = E_CU[b], E_CU[b + 1]
            truth[s:e] = logits_f64(q[s:e].transpose(0, 1)[None], w[s:e].transpose(0, 1)[None], k[b:b + 1], ks[b:b + 1])[0]
    assert truth.abs().max() < 2 ** 24 / 32 and torch.equal(truth * 32, (truth * 32).round())
    return q, w, k, ks, truth


@functools.lru_cache(maxsize=None)
def edge_mask(causal):
    """bool (total_q, S_k): the candidates of every packed row, by its own sequence's n_q(b) and N_k(b)"""
    mask = torch.zeros(E_TOTAL, E_SK, dtype=torch.bool, device=DEV)
    for b in range(E_B):
        if E_NQ[b]:
            mask[E_CU[b]:E_CU[b + 1]] = candidate_mask(E_LENS[b:b + 1], 1, E_NQ[b], E_SK, causal, DEV)[0]
    return mask


@functools.lru_cache(maxsize=None)
def edge_lists(topk, causal):
    """the restatement's lists of the truth, sequence by sequence -> int32 (total_q, topk) on the CPU"""
    truth = edge_case()[4]
    out = torch.empty(E_TOTAL, topk, dtype=torch.int32)
    for b in range(E_B):
        if E_NQ[b]:
            out[E_CU[b]:E_CU[b + 1]] = topk_lists(truth[None, E_CU[b]:E_CU[b + 1]], E_LENS[b:b + 1], topk, causal)[0]
    return out


@pytest.mark.parametrize("topk", TOPKS)
@pytest.mark.parametrize("causal", [True, False])
def test_edge_batch_of_empty_sequences_finds_every_row_s_owner(causal, topk):
    """the selection alone on given logits, then scores and selection under both score forms: lists equal to the restatement per
    sequence exactly, logits equal to it bit for bit on the candidates, and in pre-filled buffers nothing else written"""
    q, w, k, ks, truth = edge_case()
    cu, lens = cu_of(E_CU), lens_of(E_LENS)
    mask, want = edge_mask(causal), edge_lists(topk, causal)
    assert not mask[0].any() and E_LENS[EV.OWNER[0]] == 0                                 # the row of the sequence without a key
    assert (want[0] == -1).all() and (want[E_CU[8]:E_CU[9], 0] >= 0).all()
    junk = torch.where(torch.arange(E_SK, device=DEV) % 2 == 0, float("nan"), float("inf")).expand(E_TOTAL, E_SK)
    given = torch.where(mask, truth.float(), junk)
    idx, whole, sl = arena(E_TOTAL * topk, torch.int32, -77)
    idx = idx.view(E_TOTAL, topk)
    _lib.fa2_topk_indices_varlen(given, idx, cu, E_MAXQ, lens, causal=causal)
    torch.cuda.synchronize()
    assert canaries_intact(whole, sl, -77)
    assert torch.equal(idx.cpu(), want), (causal, topk, (idx.cpu() != want).nonzero()[:5].tolist())
    assert torch.equal(fa.topk_indices_varlen(given, cu, E_MAXQ, lens, topk, causal=causal).cpu(), want)
    for variant in ("idx16", "generic"):
        what = (variant, causal, topk)
        indices, logits = fa.flash_attention_mla_indexer_topk_varlen(q.to(BF16), w, k.to(BF16), cu, E_MAXQ, lens, DEV, topk=topk,
                                                                     causal=causal, k_scale=ks, variant=variant, return_logits=True)
        assert indices.shape == (E_TOTAL, topk) and logits.shape == (E_TOTAL, E_SK) and logits.dtype == F32
        zero = torch.zeros((), dtype=F64, device=DEV)
        assert torch.equal(torch.where(mask, logits.double(), zero), torch.where(mask, truth, zero)), what
        assert torch.equal(indices.cpu(), want), (what, (indices.cpu() != want).nonzero()[:5].tolist())
        # pre-filled buffers in canary arenas: non-candidates keep their bits
        lg, lg_all, lg_sl = arena(E_TOTAL * E_SK, torch.int32, NAN_PATTERN)
        ix, ix_all, ix_sl = arena(E_TOTAL * topk, torch.int32, -77)
        lg, ix = lg.view(E_TOTAL, E_SK).view(F32), ix.view(E_TOTAL, topk)
        _lib.fa2_mla_indexer_topk_varlen(q.to(BF16), w, k.to(BF16), ks, lg, ix, cu, E_MAXQ, lens, convert_triton_dtype(BF16),
                                         convert_triton_dtype(BF16), causal=causal, variant=_lib.INDEXER_VARIANTS[variant])
        torch.cuda.synchronize()
        assert canaries_intact(lg_all, lg_sl, NAN_PATTERN) and canaries_intact(ix_all, ix_sl, -77), what
        assert (lg.view(torch.int32)[~mask] == NAN_PATTERN).all(), what
        assert torch.equal(lg[mask].view(torch.int32), logits[mask].view(torch.int32)) and torch.equal(ix.cpu(), want), what
