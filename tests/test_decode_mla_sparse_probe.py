"""CPU proof that tests/mla_sparse_probe.py -- the exact-arithmetic probe tests/test_decode_mla_sparse_probe_gpu.py runs through sparse
MLA decode (fa2_fwd_kvcache_mla_sparse) -- sees what it must:

  * the lists hold distinct valid positions mixed with every kind of entry that is no key (-1, N_k(b), S_k + 5, 2^31 - 1, -2^31), one
    list has no valid entry, and where topk > 64 one has all of them behind slot 64;
  * every planted error (an index off by one, an invalid slot read as key 0, the decoy row at N_k(b) accepted, slots at and past topk
    read, the last partial 64-slot tile dropped, a slot at a split boundary taken twice or not at all, position qi answered with the
    list of qi - 1, the second head tile answered with another position's list, another sequence's list, j % page_size from the wrong
    page size, the index taken as a physical pool row) breaks a bar, computed with the reference restatement alone, in every
    (sequence, position) the plant changes -- on every case of the GPU grid it can apply to;
  * the un-planted restatement (emulate_split over the slots of the gathered rows) breaks none at any split count of the grid and at
    what num_splits = 0 resolves to.

Bars: the decode probe's (oracle/fa2_decode_probe.violations)."""
import functools

import pytest
import torch

import mla_sparse_probe as S
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@functools.lru_cache(maxsize=None)
def cache():
    return S.latent_cache()


def test_lists_hold_what_they_must():
    assert S.LENS == (0, 1, 63, 64, 65, 1000, 2049, 2560) and S.S_K == 2560 and S.SPLITS == (0, 1, 3, 16, 128)
    assert {c[0] for c in S.CONFIGS} == {16, 40, 64, 128} and {c[1] for c in S.CONFIGS} == {1, 2, 3}
    assert {c[2] for c in S.CONFIGS} == {1, 63, 64, 65, 200, 2048}
    kinds = set()
    for H, n_q, topk in S.CONFIGS:
        idx = S.lists(n_q, topk)
        ok = S.valid(idx)
        assert idx.shape == (S.B, 1, n_q, topk) and idx.dtype == torch.int32
        assert not ok[S.EMPTY_B, 0, 0].any() and not ok[0].any()                  # a list with none; the empty sequence
        for b, nk in enumerate(S.LENS):
            for qi in range(n_q):
                j = idx[b, 0, qi][ok[b, 0, qi]]
                assert j.unique().numel() == j.numel()                            # distinct
                kinds |= set(idx[b, 0, qi][~ok[b, 0, qi]].tolist()) - {nk}
                if (idx[b, 0, qi] == nk).any():
                    kinds.add("nk")
        if topk > 64:
            late = ok[S.LATE_B, 0, 0]
            assert late[64:].any() and not late[:64].any()                        # all valid entries behind slot 64
            assert ok.reshape(-1, topk)[:, :64].any() and ok.sum() > ok.numel() // 4
    assert kinds >= {-1, "nk", S.S_K + 5, 2 ** 31 - 1, -2 ** 31}


def _auto(H, n_q, topk, dtype):
    return _lib.kvcache_mla_sparse_num_splits(S.B, H, 1, n_q, topk, 576, 512, convert_triton_dtype(dtype))


@pytest.mark.parametrize("k", range(len(S.CONFIGS)))
def test_unplanted_restatement_breaks_no_bar(k):
    H, n_q, topk = S.CONFIGS[k]
    idx = S.lists(n_q, topk)
    K, keep = S.gather(cache()[:, 0], idx, S.valid(idx), H)
    for uniform in (False, True):
        Q = S.gathered_queries(H, n_q, uniform)
        for dt in (BF16, F16, F32):
            if dt != BF16 and uniform:
                continue                                                          # (the count ratios: once)
            ref = S.truth(Q, K, keep, dt)
            for n in sorted(set(S.SPLITS[1:]) | {_auto(H, n_q, topk, dt)}):
                if dt != BF16 and n not in (1, 3, 128):
                    continue
                O, L = S.restate(Q, K, keep, n, dt)
                assert O.shape == (S.B * n_q, 1, H, 512)
                v = D.violations(O, L, *ref, dt, n > 1)
                assert not v, (S.CONFIGS[k], uniform, dt, n, v)


@pytest.mark.parametrize("k", range(len(S.CONFIGS)))
def test_every_plant_breaks_a_bar_in_every_sequence_and_position_it_changes(k):
    """The planted restatement against the truth, each (sequence, position) judged on its own.  A plant changes one where the fp64
    truth of the planted computation differs from the un-planted truth; the scored probe must see it there, or the uniform one."""
    H, n_q, topk = S.CONFIGS[k]
    KV = cache()
    idx = S.lists(n_q, topk)
    K, keep = S.gather(KV[:, 0], idx, S.valid(idx), H)
    P = S.B * n_q
    seen_somewhere = set()
    for dt in (BF16, F16, F32):
        probes = {}
        for uniform in (False, True):
            Q = S.gathered_queries(H, n_q, uniform)
            probes[uniform] = (Q, S.truth(Q, K, keep, dt))
        for name in S.PLANTS:
            changed = torch.zeros(P, dtype=torch.bool)
            caught = torch.zeros(P, dtype=torch.bool)
            for uniform, (Q, (O_ref, L_ref)) in probes.items():
                got = S.planted_outputs(name, lambda q, kk, kp: S.truth(q, kk, kp, dt), Q, KV, idx, H)
                if got is None:
                    continue
                O_t, L_t = got
                ch = ((O_t != O_ref).reshape(P, -1).any(-1) | (L_t != L_ref).reshape(P, -1).any(-1))
                if not ch.any():
                    continue
                O_p, L_p = S.planted_outputs(name, lambda q, kk, kp: S.restate(q, kk, kp, 1, dt), Q, KV, idx, H)
                hit = D.violated(O_p, L_p, O_ref, L_ref, dt, False)
                if dt == F32:                                                     # every configuration runs split as well
                    hit &= D.violated(O_p, L_p, O_ref, L_ref, dt, True)
                changed |= ch
                caught |= ch & hit
            missed = [(p // n_q, p % n_q) for p in torch.nonzero(changed & ~caught).flatten().tolist()]
            assert not missed, (S.CONFIGS[k], name, dt, missed)
            if changed.any():
                seen_somewhere.add(name)
    # on this configuration every plant that can apply is a real error somewhere
    expect = set(S.PLANTS)
    if topk % 64 == 0:
        expect -= {"past_topk_read", "drop_last_partial"}
    if D.split_chunk(topk, 3) >= topk:
        expect -= {"boundary_twice", "boundary_skipped"}
    if n_q < 2:
        expect -= {"previous_position", "second_tile_other_position"}
    if H <= 64:
        expect.discard("second_tile_other_position")
    nk = torch.tensor(S.LENS).view(S.B, 1, 1, 1)
    if not ((idx == nk) & (idx < S.S_K)).any():
        expect.discard("decoy_accepted")  # (eight lists of one slot: none draws the entry N_k(b))
    assert expect <= seen_somewhere, (S.CONFIGS[k], expect - seen_somewhere)


def test_every_plant_is_a_real_error_on_the_grid():
    """each plant has configurations it applies to: a partial last tile, a split boundary inside the list, two positions, two head tiles"""
    assert any(t % 64 for _, _, t in S.CONFIGS) and any(D.split_chunk(t, 3) < t for _, _, t in S.CONFIGS)
    assert any(n >= 2 and H > 64 for H, n, _ in S.CONFIGS)
    nk = torch.tensor(S.LENS).view(S.B, 1, 1, 1)
    with_decoy = [c for c in S.CONFIGS if ((S.lists(c[1], c[2]) == nk) & (nk < S.S_K)).any()]
    assert len(with_decoy) >= len(S.CONFIGS) - 1  # the entry N_k(b) is drawn on every configuration but the one-slot one
