"""The selection of the MLA indexer alone (fa2_topk_indices) on given logits: exact equality of `indices` with the restatement
(tests/mla_indexer_restatement.py) -- no tolerance enters a selection.  Entries that are no candidates hold NaN and +inf, the output
sits in a canary arena."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from mla_indexer_restatement import candidate_mask, counts, topk_lists
from test_decode_gpu import arena, canaries_intact, lens_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S_K = 2560
LENS = [0, 1, 63, 64, 65, 1000, 2049, S_K]
B = len(LENS)
KINDS = ("normal", "ints7", "equal", "zeros", "special", "lsb", "negative")
CANARY = -77


def make_logits(kind, N_q, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, N_q, S_K)
    if kind == "normal":
        x = torch.randn(shape, generator=g)
    elif kind == "ints7":  # seven values: ties everywhere, the tie rule decides most of the list
        x = torch.randint(-3, 4, shape, generator=g).float()
    elif kind == "equal":
        x = torch.full(shape, 1.5)
    elif kind == "zeros":  # +0.0 and -0.0 compare equal
        x = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    elif kind == "special":  # NaN and both infinities planted
        x = torch.randn(shape, generator=g)
        r = torch.rand(shape, generator=g)
        x[r < 0.05] = float("nan")
        x[(r >= 0.05) & (r < 0.10)] = float("inf")
        x[(r >= 0.10) & (r < 0.15)] = -float("inf")
    elif kind == "lsb":  # values that differ only in their lowest mantissa bit
        x = (torch.full(shape, 0x3f800000, dtype=torch.int32) + torch.randint(0, 2, shape, generator=g, dtype=torch.int32)).view(torch.float32)
    else:  # all negative
        x = -torch.randn(shape, generator=g).abs() - 0.1
    return x


@functools.lru_cache(maxsize=None)
def case(kind, N_q, causal):
    """the logits on the device with NaN / +inf behind every row's candidates, and the candidate mask: made once per (kind, N_q, causal)"""
    x = make_logits(kind, N_q, 11 * KINDS.index(kind) + N_q)
    mask = candidate_mask(LENS, B, N_q, S_K, causal)
    junk = torch.where(torch.arange(S_K) % 2 == 0, torch.tensor(float("nan")), torch.tensor(float("inf"))).expand(B, N_q, S_K)
    return torch.where(mask, x, junk).to(DEV), mask


@functools.lru_cache(maxsize=None)
def truth(kind, N_q, causal, topk):
    return topk_lists(case(kind, N_q, causal)[0], LENS, topk, causal)


def select(logits, lens, topk, causal):
    """fa2_topk_indices into a canary arena -> (indices, arena, slice)"""
    nb, nq, _ = logits.shape
    idx, whole, sl = arena(nb * nq * topk, torch.int32, CANARY)
    idx = idx.view(nb, nq, topk)
    _lib.fa2_topk_indices(logits, idx, lens, causal=causal)
    torch.cuda.synchronize()
    return idx, whole, sl


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("topk", [1, 63, 64, 65, 2048])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("N_q", [1, 3])
def test_selection_equals_the_restatement(N_q, causal, topk, kind):
    logits, mask = case(kind, N_q, causal)
    want = truth(kind, N_q, causal, topk)
    idx, whole, sl = select(logits, lens_of(LENS), topk, causal)
    assert canaries_intact(whole, sl, CANARY)
    got = idx.cpu()
    assert torch.equal(got, want), (kind, N_q, causal, topk, (got != want).nonzero()[:5].tolist())
    # no list names an entry that is no candidate; every list ascends; it holds min(topk, n) keys
    n = torch.tensor(counts(LENS, B, N_q, S_K, causal))
    listed = got >= 0
    assert (got[listed] < n[..., None].expand_as(got)[listed]).all()
    assert torch.equal(listed.sum(-1), n.clamp(max=topk))
    if topk > 1:
        assert ((got[..., 1:] > got[..., :-1]) | (got[..., 1:] < 0)).all()
    # the Python surface is the same call
    assert torch.equal(fa.topk_indices(logits, lens_of(LENS), topk, causal=causal).cpu(), want)


@pytest.mark.parametrize("kind", ["normal", "ints7", "special"])
def test_strided_logits_give_the_bytes_of_their_contiguous_copy(kind):
    N_q, topk = 3, 64
    logits, _ = case(kind, N_q, True)
    lens = lens_of(LENS)
    want = truth(kind, N_q, True, topk)
    wide = torch.full((B, N_q, 2 * S_K + 3), float("inf"), device=DEV)
    wide[..., 1:2 * S_K + 1:2] = logits
    swapped = logits.transpose(0, 1).contiguous().transpose(0, 1)  # (B, N_q, S_k) over an (N_q, B, S_k) buffer
    for view in (wide[..., 1:2 * S_K + 1:2], swapped):
        assert not view.is_contiguous()
        idx, whole, sl = select(view, lens, topk, True)
        assert canaries_intact(whole, sl, CANARY) and torch.equal(idx.cpu(), want)
    # ... and a strided OUTPUT: every second slot of a wider row
    out = torch.full((B, N_q, 2 * topk), CANARY, dtype=torch.int32, device=DEV)
    _lib.fa2_topk_indices(logits, out[..., ::2], lens, causal=True)
    assert torch.equal(out[..., ::2].cpu(), want) and (out[..., 1::2] == CANARY).all()
    # two-dimensional logits with N_q given, and lens = None: every row has S_k candidates (non-causal)
    flat = make_logits(kind, N_q, 5).to(DEV)
    assert torch.equal(fa.topk_indices(flat.flatten(0, 1), None, topk, N_q=N_q, causal=False).cpu(), topk_lists(flat, None, topk, False))


def test_same_logits_same_bytes():
    logits, _ = case("ints7", 3, True)
    first = select(logits, lens_of(LENS), 2048, True)[0].clone()
    for _ in range(3):
        assert torch.equal(select(logits, lens_of(LENS), 2048, True)[0], first)
