"""CPU proof that tests/mla_prefill_probe.py -- the exact-arithmetic probe tests/test_mla_prefill_probe_gpu.py runs through the
packed forward at d = 192 / d_v = 128 (fa2_fwd_varlen_dv) -- sees what it must:

  * the inputs are exact in every dtype, scores are integers in [0, 8], each of the 12 k-steps carries one score column, four of
    them in columns 128..191, every row's score draws on both K images, and the value code is two ones per key;
  * the un-planted restatement (a valid fp32 implementation) breaks no bar on any case of the grid;
  * every planted error (PLANTS) breaks a bar, computed with the restatement alone, in every sequence the plant changes -- a
    sequence is changed where the fp64 truth of the planted computation differs from the un-planted truth; the scored probe must
    see it there, or the uniform one.

Bars: oracle.fa2_mask_probe.violations -- 16-bit I/O one output ulp on O and L, exact zeros, exact empty rows; float32 4 ulps."""
import functools

import pytest
import torch

import mla_prefill_probe as M

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
CASES = M.cases()


@functools.lru_cache(maxsize=None)
def probe(h_kv, uniform):
    return M.inputs(h_kv, uniform)


def test_probe_layout_and_exactness():
    sc = M.SCORE_COLS
    assert len(sc) == 12 and [c // 16 for c in sc] == list(range(12))            # one per k-step of a 32x32x16 MFMA
    assert sum(c >= 128 for c in sc) == 4 and sum(c < 128 for c in sc) == 8       # four of them in the rotary image
    assert M.LQ == [0, 1, 31, 127, 128, 129, 300, 40] and M.LK == [5, 1, 65, 31, 128, 257, 300, 0]
    for h_kv in M.H_KVS:
        Q, K, V = probe(h_kv, False)
        assert Q.shape == (sum(M.LQ), 4, 192) and K.shape == (sum(M.LK), h_kv, 192) and V.shape == (sum(M.LK), h_kv, 128)
        for t in (Q, K, V):
            for dt in (F16, BF16, F32):
                assert torch.equal(t.to(dt).double(), t)
        rest = torch.ones(192, dtype=torch.bool)
        rest[torch.tensor(sc)] = False
        assert (K[..., rest] == 0).all() and (Q[..., rest] == 0).all() and K.max() == 4 and K.min() == 0
        assert (Q[..., :128].sum(-1) == 1).all() and (Q[..., 128:].sum(-1) == 1).all()      # one nope step, one rotary step per row
        assert (Q.sum((0, 1))[torch.tensor(sc)] > 0).all()                                    # every k-step is some row's
        assert not torch.equal(Q[:-32], Q[32:]) and not torch.equal(Q[:-1], Q[1:])
        S = torch.einsum("qhd,khd->hqk", Q, M.expand(K, h_kv))
        assert S.min() == 0 and S.max() == 8 and torch.equal(S, S.round())
        assert torch.equal(V.sum(-1), torch.full(V.shape[:2], 2.0)) and V.max() <= 2 and (V[..., :64].sum(-1) == 1).all()
        assert (probe(h_kv, True)[0] == 0).all()
    # exact fp32 sums: at most 300 visible keys of weight <= 2^8 in units of 2^-8
    assert 2 * max(M.LK) * 2 ** 16 < 2 ** 24 * 4


@pytest.mark.parametrize("h_kv,causal,window", CASES)
def test_unplanted_restatement_breaks_no_bar(h_kv, causal, window):
    keep = M.keep_of(causal, window)
    for uniform in (False, True):
        Q, K, V = probe(h_kv, uniform)
        for dt in (BF16, F16, F32):
            ref = M.reference(Q, K, V, h_kv, keep, dt)
            O, L = M.reference(Q, K, V, h_kv, keep, dt, M.emulate)
            assert O.shape == (sum(M.LQ), 4, 128) and L.shape == (4, sum(M.LQ))
            v = M.violations_of(O, L, *ref, dt)
            assert not v, (uniform, dt, v)


@pytest.mark.parametrize("h_kv,causal,window", CASES)
def test_every_plant_breaks_a_bar_in_every_sequence_it_changes(h_kv, causal, window):
    keep = M.keep_of(causal, window)
    seen = set()
    for dt in (BF16, F32):
        probes = {}
        for uniform in (False, True):
            Q, K, V = probe(h_kv, uniform)
            probes[uniform] = (Q, K, V, M.reference(Q, K, V, h_kv, keep, dt))
        for name in M.PLANTS:
            missed, runs = [], {}
            for b, rows in enumerate(M.sequences()):
                changed = caught = False
                for uniform, (Q, K, V, (O_ref, L_ref)) in probes.items():
                    if uniform not in runs:  # (the planted truth and the planted restatement: once per plant and probe)
                        runs[uniform] = (M.planted(name, Q, K, V, h_kv, causal, window, dt),
                                         M.planted(name, Q, K, V, h_kv, causal, window, dt, M.emulate))
                    (O_t, L_t), (O_p, L_p) = runs[uniform]
                    if torch.equal(O_t[rows], O_ref[rows]) and torch.equal(L_t[:, rows], L_ref[:, rows]):
                        continue
                    changed = True
                    caught |= bool(M.violations_of(O_p, L_p, O_ref, L_ref, dt, rows))
                if changed:
                    seen.add(name)
                    if not caught:
                        missed.append((M.LQ[b], M.LK[b]))
            assert not missed, (name, dt, missed)
    # on this case every plant that can apply is a real error in some sequence
    expect = set(M.PLANTS)
    if h_kv in (4, 1):  # (h % H_kv is h // g there)
        expect.discard("kv_head_mod")
    if window is None or window[0] < 0:
        expect.discard("left_minus_one")
    if not causal and (window is None or window[1] < 0):
        expect.discard("right_plus_one")
    if not causal and window is None:
        expect.discard("top_left")
    assert expect <= seen, expect - seen


def test_every_plant_is_a_real_error_on_the_grid():
    assert any(hk < 4 for hk, _, _ in CASES) and any(c for _, c, _ in CASES) and any(w and w[0] >= 0 for _, _, w in CASES)
    assert any(nk % 64 for nk in M.LK) and any(nq > 32 for nq in M.LQ)
