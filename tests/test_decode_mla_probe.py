"""CPU proof that tests/mla_probe.py -- the exact-arithmetic probe tests/test_decode_mla_probe_gpu.py runs through MLA decode
(fa2_fwd_kvcache_mla: d = 576, d_v = 512, V the first 512 columns of K) -- sees what it must:

  * the latent rows are exact in every dtype, scores are integers in [0, 8], every 16-column k-step and both sides of column 512
    carry a score column, Q is zero on the value code;
  * every planted error (the rotary columns or one k-step left out of the score, V taken from columns 64..575, two 128-column value
    blocks exchanged, the second 64-row tile answered with the first one's rows, rows r and r + 32 exchanged, a stale row leaking in,
    the last partial tile dropped, top-left alignment) breaks a bar, computed with the reference restatement alone, in every sequence
    the plant changes -- on every case of the GPU grid, no case skipped;
  * the un-planted restatement breaks none, under every split count of the grid and what num_splits = 0 resolves to.

Bars: the decode probe's (oracle/fa2_decode_probe.violations) -- 16-bit I/O one output ulp on O and L, exact zeros, exact empty
rows at any num_splits; float32 its 4 ulps unsplit and SPLIT_FP32_ULPS split."""
import functools

import pytest
import torch

import mla_probe as M
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
B = len(M.LENS)


@functools.lru_cache(maxsize=None)
def cache():
    return M.latent_cache()


def test_probe_layout_and_exactness():
    KV = cache()
    assert KV.shape == (B, 1, M.S_K, 576) and M.D_QK == 576 and M.D_V == 512
    sc = set(M.SCORE_COLS)
    assert len(sc) == 36 and {c // 16 for c in sc} == set(range(36))             # one per k-step of a 32x32x16 MFMA
    assert sum(c >= 512 for c in sc) == 4 and sum(c < 512 for c in sc) == 32      # both sides of column 512
    assert len({c % 16 for c in sc}) == 16                                        # every position inside a k-step
    assert not sc & set(M.VALUE_COLS) and len(M.VALUE_COLS) == 480 and max(M.VALUE_COLS) < 512
    assert KV.min() == 0 and KV.max() == 8 and torch.equal(KV, KV.round())
    for dt in (F16, BF16, F32):
        assert torch.equal(KV.to(dt).double(), KV)
    vc = torch.tensor(M.VALUE_COLS)
    assert torch.equal(KV[..., vc].sum(-1), torch.full((B, 1, M.S_K), 2.0)) and KV[..., vc].max() == 1   # two ones per key
    rest = torch.ones(576, dtype=torch.bool)
    rest[torch.tensor(M.SCORE_COLS)] = False
    assert (KV[..., 512:][..., rest[512:]] == 0).all()                           # the rotary side holds score columns only
    for b, nk in enumerate(M.LENS):
        assert (KV[b, :, nk:][..., torch.tensor(M.SCORE_COLS)] == 8).all()       # decoys: the largest score
    for H, n_q, _, _ in M.CONFIGS:
        for uniform in (False, True):
            Q = M.queries(H, n_q, uniform)
            assert (Q[..., vc] == 0).all()                                       # the value code never reaches a score
            S = Q @ KV.transpose(-1, -2)
            assert S.min() == 0 and S.max() == (0 if uniform else 8) and torch.equal(S, S.round())
        if H * n_q >= 36:
            assert (M.queries(H, n_q).sum(-2) > 0).sum(-1).eq(36).all()                          # every score column is some row's
    # the overlap columns stay exact: sums of P K in units of 2^-8 below 2^24
    assert 8 * M.S_K * 2 ** 8 < 2 ** 24
    # the configurations cover one row tile, two, four, and a last partial tile
    assert {-(-H * n // 64) for H, n, _, _ in M.CONFIGS} == {1, 2, 4} and any((H * n) % 64 for H, n, _, _ in M.CONFIGS)


def _auto(H, n_q, dtype):
    return _lib.kvcache_mla_num_splits(B, H, 1, n_q, M.S_K, 576, 512, convert_triton_dtype(dtype))


@pytest.mark.parametrize("k", range(len(M.CONFIGS)))
def test_unplanted_restatement_breaks_no_bar(k):
    H, n_q, causal, window = M.CONFIGS[k]
    KV = cache()
    keep = M.decode_keep(H, n_q, causal, window)
    for uniform in (False, True):
        Q = M.queries(H, n_q, uniform)
        for dt in (BF16, F16, F32):
            if dt != BF16 and uniform:
                continue                                                        # (the count ratios: once)
            ref = M.mla_truth(Q, KV, keep, dt)
            for n in sorted(set(M.SPLITS[1:]) | {_auto(H, n_q, dt)}):
                if dt != BF16 and n not in (1, 3, 128):
                    continue
                O, L = M.restate(Q, KV, M.value_of(KV), keep, M.LENS, n, dt)
                assert O.shape[-1] == 512
                v = M.violations(O, L, *ref, dt, n > 1)
                assert not v, (M.CONFIGS[k], uniform, dt, n, v)


@pytest.mark.parametrize("k", range(len(M.CONFIGS)))
def test_every_plant_breaks_a_bar_in_every_sequence_it_changes(k):
    """The planted restatement against the truth, each sequence judged on its own.  A plant changes a sequence where the fp64 truth
    of the planted computation differs from the un-planted truth; the scored probe must see it there, or the uniform one."""
    H, n_q, causal, window = M.CONFIGS[k]
    KV = cache()
    keep = M.decode_keep(H, n_q, causal, window)
    seen_somewhere = set()
    for dt in (BF16, F16, F32):
        probes = {}
        for uniform in (False, True):
            Q = M.queries(H, n_q, uniform)
            probes[uniform] = (Q, M.mla_truth(Q, KV, keep, dt))
        for name in M.PLANTS:
            changed = torch.zeros(B, dtype=torch.bool)
            caught = torch.zeros(B, dtype=torch.bool)
            for uniform, (Q, (O_ref, L_ref)) in probes.items():
                O_t, L_t = M.planted(name, Q, KV, H, n_q, causal, window, lambda q, kk, v, kp: M.truth(q, kk, v, kp, dt))
                ch = ((O_t != O_ref).reshape(B, -1).any(-1) | (L_t != L_ref).reshape(B, -1).any(-1))
                if not ch.any():
                    continue
                O_p, L_p = M.planted(name, Q, KV, H, n_q, causal, window,
                                     lambda q, kk, v, kp: M.restate(q, kk, v, kp, M.LENS, 1, dt))
                hit = D.violated(O_p, L_p, O_ref, L_ref, dt, False)
                if dt == F32:                                                   # every configuration runs split as well
                    hit &= D.violated(O_p, L_p, O_ref, L_ref, dt, True)
                changed |= ch
                caught |= ch & hit
            missed = [M.LENS[b] for b in torch.nonzero(changed & ~caught).flatten().tolist()]
            assert not missed, (M.CONFIGS[k], name, dt, missed)
            if changed.any():
                seen_somewhere.add(name)
    # on this configuration every plant that can apply is a real error in some sequence
    expect = set(M.PLANTS)
    if H * n_q <= 64:
        expect.discard("second_tile_repeats_first")
    if H * n_q <= 32:
        expect.discard("plus32")
    if not causal and window is None:
        expect.discard("top_left")
    assert expect <= seen_somewhere, (M.CONFIGS[k], expect - seen_somewhere)


def test_every_plant_is_a_real_error_on_the_grid():
    """second_tile_repeats_first needs two row tiles, plus32 more than 32 rows, top_left a mask: each has its configurations"""
    assert any(H * n > 64 for H, n, _, _ in M.CONFIGS) and any(c or w for _, _, c, w in M.CONFIGS)
