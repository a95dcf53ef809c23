"""The split-row selection of the MLA indexer (fa2_topk_indices_split, num_splits >= 2) on given logits: exact equality of `indices`
with the restatement (tests/mla_indexer_restatement.py) AND with the one-workgroup kernel (num_splits = 1).  3,000 keys in chunks of
1,024: lengths on both sides of every chunk seam, the seven kinds of logits of tests/test_mla_indexer_topk_gpu.py (all-equal and
seven-value rows put the threshold's ties across a seam).  The output sits in a canary arena, the workspace is pre-filled with 0xFF
bytes, and the fixed form's logits hold NaN and +inf behind every row's candidates."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from mla_indexer_restatement import candidate_mask, topk_lists
from test_decode_gpu import arena, canaries_intact, lens_of
from test_mla_indexer_topk_gpu import KINDS, make_logits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S_K, B = 3000, 3
LENS = ([0, 1024, 2999], [1, 1025, 3000], [1023, 2047, 2049])
TOPKS = (1, 64, 65, 2048)
CANARY = -77


def raw(kind, N_q, group):
    """(B, N_q, S_K) logits of `kind`: the fixed selection test's generator, its elements laid out anew"""
    x = make_logits(kind, N_q, 7 * KINDS.index(kind) + group).transpose(0, 1).reshape(N_q, -1)
    return x[:, :B * S_K].reshape(N_q, B, S_K).transpose(0, 1)


@functools.lru_cache(maxsize=None)
def case(kind, N_q, group, causal):
    """raw() on the device with NaN / +inf behind every row's candidates"""
    x = raw(kind, N_q, group)
    junk = torch.where(torch.arange(S_K) % 2 == 0, torch.tensor(float("nan")), torch.tensor(float("inf"))).expand(B, N_q, S_K)
    return torch.where(candidate_mask(LENS[group], B, N_q, S_K, causal), x, junk).to(DEV)


def select(logits, lens, topk, causal, splits, out=None):
    """fa2_topk_indices_split over a workspace of 0xFF bytes, into a canary arena (or `out`) -> (indices, arena, slice)"""
    nb, nq, _ = logits.shape
    idx, whole, sl = arena(nb * nq * topk, torch.int32, CANARY)
    idx = idx.view(nb, nq, topk) if out is None else out
    ws = torch.full((_lib.topk_workspace_bytes(nb * nq, splits),), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.fa2_topk_indices(logits, idx, lens_of(lens), causal=causal, num_splits=splits, workspace=ws)
    torch.cuda.synchronize()
    return idx, whole, sl


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("N_q", [1, 3])
def test_split_selection_equals_the_restatement_and_the_one_workgroup_kernel(N_q, causal, kind):
    for group, lens in enumerate(LENS):
        logits = case(kind, N_q, group, causal)
        for topk in TOPKS:
            want = topk_lists(logits, lens, topk, causal)
            assert torch.equal(fa.topk_indices(logits, lens_of(lens), topk, causal=causal, num_splits=1).cpu(), want)
            for splits in (2, 3) + ((256,) if topk == 65 else ()):  # (256: clamped to the three chunks)
                idx, whole, sl = select(logits, lens, topk, causal, splits)
                got = idx.cpu()
                assert canaries_intact(whole, sl, CANARY)
                assert torch.equal(got, want), (kind, N_q, causal, lens, topk, splits, (got != want).nonzero()[:5].tolist())
            assert torch.equal(fa.topk_indices(logits, lens_of(lens), topk, causal=causal, num_splits=3).cpu(), want)  # the Python surface


@pytest.mark.parametrize("kind", ["normal", "ints7", "special"])
def test_strided_and_misaligned_logits_give_the_bytes_of_the_contiguous_call(kind):
    N_q, topk, lens = 3, 64, LENS[1]
    logits = case(kind, N_q, 1, True)
    want = select(logits, lens, topk, True, 3)[0].clone()
    assert torch.equal(want.cpu(), topk_lists(logits, lens, topk, True))
    wide = torch.full((B, N_q, 2 * S_K + 3), float("inf"), device=DEV)
    wide[..., 1:2 * S_K + 1:2] = logits  # a column stride of 2: scalar loads
    odd = torch.full((B, N_q, S_K + 1), float("inf"), device=DEV)
    odd[..., 1:] = logits  # unit column stride, rows 3,001 floats apart from a 4-byte offset: every head and tail of the 16-byte loads
    for view in (wide[..., 1:2 * S_K + 1:2], odd[..., 1:]):
        assert not view.is_contiguous()
        idx, whole, sl = select(view, lens, topk, True, 3)
        assert canaries_intact(whole, sl, CANARY) and torch.equal(idx, want)
    out = torch.full((B, N_q, 2 * topk), CANARY, dtype=torch.int32, device=DEV)  # a strided output: every second slot
    select(logits, lens, topk, True, 2, out=out[..., ::2])
    assert torch.equal(out[..., ::2], want) and (out[..., 1::2] == CANARY).all()


@pytest.mark.parametrize("kind,causal", [("ints7", True), ("equal", False), ("normal", True)])
def test_packed_rows_with_an_empty_sequence_and_a_row_no_sequence_owns(kind, causal):
    nq, lens, topk = [2, 0, 3], [2999, 500, 1025], 64
    cu = torch.tensor([0, 2, 2, 5], dtype=torch.int32, device=DEV)  # six packed rows, the last one nobody's
    logits = raw(kind, 2, 1).flatten(0, 1).to(DEV)
    want = torch.full((6, topk), CANARY, dtype=torch.int32)
    for b, (s, e) in enumerate(((0, 2), (2, 2), (2, 5))):
        if e > s:
            want[s:e] = topk_lists(logits[None, s:e], lens[b:b + 1], topk, causal)[0]
    for splits in (1, 3):
        idx, whole, sl = arena(6 * topk, torch.int32, CANARY)
        ws = torch.full((_lib.topk_workspace_bytes(6, 3),), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.fa2_topk_indices_varlen(logits, idx.view(6, topk), cu, 3, lens_of(lens), causal=causal, num_splits=splits, workspace=ws)
        assert canaries_intact(whole, sl, CANARY) and torch.equal(idx.view(6, topk).cpu(), want), splits
    assert torch.equal(fa.topk_indices_varlen(logits, cu, 3, lens_of(lens), topk, causal=causal, num_splits=3)[:5].cpu(), want[:5])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn], ids=str)
def test_fused_wrappers_with_a_split_selection_equal_the_fused_call(dtype):
    g = torch.Generator().manual_seed(5)
    q, w, k = torch.randn(2, 16, 2, 128, generator=g), torch.rand(2, 16, 2, generator=g), torch.randn(2, S_K, 128, generator=g)
    fp8 = dtype != torch.bfloat16
    q, k, ks = q.to(dtype).to(DEV), k.to(dtype).to(DEV), torch.ones(2, S_K, device=DEV) if fp8 else None
    lens, cu = [2049, 3000], torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    one, logits = fa.flash_attention_mla_indexer_topk(q, w.to(DEV), k, lens_of(lens), DEV, topk=64, k_scale=ks, select_splits=1, return_logits=True)
    assert torch.equal(one.cpu(), topk_lists(logits, lens, 64, True))
    assert torch.equal(fa.flash_attention_mla_indexer_topk(q, w.to(DEV), k, lens_of(lens), DEV, topk=64, k_scale=ks, select_splits=3), one)
    qp, wp = q.transpose(1, 2).flatten(0, 1), w.to(DEV).transpose(1, 2).flatten(0, 1)
    packed = [fa.flash_attention_mla_indexer_topk_varlen(qp, wp, k, cu, 2, lens_of(lens), DEV, topk=64, k_scale=ks, select_splits=splits)
              for splits in (1, 3)]
    assert torch.equal(packed[0], packed[1]) and packed[0].shape == (4, 64)


def test_captured_in_a_graph_every_replay_equals_the_eager_call():
    N_q, topk, lens = 3, 2048, lens_of(LENS[1])
    static = case("normal", N_q, 1, True).clone()
    out = torch.empty((B, N_q, topk), dtype=torch.int32, device=DEV)
    ws = torch.full((_lib.topk_workspace_bytes(B * N_q, 3),), 0xFF, dtype=torch.uint8, device=DEV)
    _lib.fa2_topk_indices(static, out, lens, causal=True, num_splits=3, workspace=ws)  # (the kernels are loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.fa2_topk_indices(static, out, lens, causal=True, num_splits=3, workspace=ws)
    for kind in ("ints7", "equal", "normal", "special"):
        static.copy_(case(kind, N_q, 1, True))
        out.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, select(static, LENS[1], topk, True, 3)[0]), kind
        assert torch.equal(out.cpu(), topk_lists(static, LENS[1], topk, True)), kind
