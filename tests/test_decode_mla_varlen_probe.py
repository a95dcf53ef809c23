"""CPU proof that tests/mla_varlen_probe.py -- the exact-arithmetic probe tests/test_decode_mla_varlen_probe_gpu.py runs through packed
queries over the latent cache (fa2_fwd_kvcache_mla_varlen) -- sees what it must, on the ragged batch and the configurations of
tests/test_decode_mla_varlen_gpu.py:

  * the un-planted restatement (mla_probe.restate, one sequence at a time with its own n_q(b)) breaks no bar, for every
    configuration, scored and uniform, in bf16, f16 and f32, at every split count of SPLITS and at what num_splits = 0 resolves to;
    its worst float32 error in fp32 ulps is measured and printed;
  * every planted error -- the ten of the packed layout (rows head-major inside the group, the mask row taken in the tile, the shift
    from max_seqlen_q, a neighbour's cu_seqlens_q offset or N_k, the first key tile or the last key of a row tile's own band not
    read, a row tile answered by the rotated one, rows rho and rho + 32 exchanged) and mla_probe's own eight, per sequence -- breaks
    a bar in every sequence whose truth it changes, in every dtype, on the scored or on the uniform probe.  No exclusions.  The test
    prints, per plant, in how many (configuration, sequence) pairs it changed anything, and one row the bars catch it in;
  * the helper's pieces are mla_probe's own, and packing and grouping are inverse.

Bars: oracle/fa2_decode_probe.violations -- 16-bit I/O one output ulp on O and L, exact zeros, exact empty rows at any num_splits;
float32 its 4 ulps unsplit and SPLIT_FP32_ULPS split."""
import functools

import pytest
import torch

import mla_probe as M
import mla_varlen_probe as V
from flash_attention_dlrs_amd import _lib
from oracle import fa2_decode_probe as D
from oracle.fa2_bwd_arith import c_log2e
from oracle.fa2_mask_probe import _bars
from test_decode_mla_varlen_host import _formula

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = (BF16, F16, F32)
SEQS = [b for b in range(V.B) if V.N_Q[b]]
name_of = lambda dt: str(dt)[6:]


def _auto(g, h_kv, dtype):
    return _lib.kvcache_mla_varlen_num_splits(V.B, g * h_kv, h_kv, V.TOTAL, V.MAX_Q, V.S_K, 576, 512,
                                              {BF16: _lib.FA2_DTYPE_BF16, F16: _lib.FA2_DTYPE_F16, F32: _lib.FA2_DTYPE_F32}[dtype])


def split_chunk(n_k, num_splits):
    return ((n_k + num_splits - 1) // num_splits + 63) & ~63


def test_the_probe_s_batch_holds_every_class_of_length():
    """the classes tests/test_decode_mla_varlen_gpu.py states for its batch, for the probe's"""
    pairs = list(zip(V.N_Q, V.N_K))
    assert max(V.N_Q) == V.MAX_Q == 70 and V.TOTAL == 163 and V.S_K == 2560 and V.CU[-1] == V.TOTAL and len(V.CU) == V.B + 1
    assert any(nq == 0 for nq in V.N_Q)                                                   # a sequence with no query
    assert any(nq > 0 and nk == 0 for nq, nk in pairs)                                    # N_k = 0
    assert any(0 < nk < nq for nq, nk in pairs)                                           # N_k < n_q: rows without a key under causal
    assert any(nq == nk == 64 for nq, nk in pairs)                                        # pure prefill of one whole key tile
    assert any(nk > nq > 0 and (nk - nq) // 64 != (nk - 1) // 64 for nq, nk in pairs)     # the chunk straddles a 64-key tile edge
    assert any(nk == V.S_K for nk in V.N_K)
    used = set(V.SPLITS[2:]) | {V.split_formula(g, h_kv) for g, h_kv, _, _ in V.CONFIGS}
    for n in sorted(used - {1}):                                                          # a split edge inside a chunk, at every split count
        assert any(nk - nq < s * split_chunk(nk, n) < nk for nq, nk in pairs if nq > 1 for s in range(1, n)), n
    for g in {c[0] for c in V.CONFIGS}:                                                   # more than one row tile, a partly filled last one
        assert g * V.MAX_Q > 64 or g == 1
    assert any((g * nq) % 64 for g, _, _, _ in V.CONFIGS for nq in V.N_Q)
    assert {c[0] for c in V.CONFIGS} == {1, 5, 16, 40, 64, 128} and (16, 2) in {c[:2] for c in V.CONFIGS}
    assert {c[3] for c in V.CONFIGS} == set(V.WINDOWS) and {c[2] for c in V.CONFIGS} == {False, True}
    # a tile spans many positions, exactly one, is smaller than one position's heads, cuts a position
    assert {64 % g == 0 for g, _, _, _ in V.CONFIGS} == {False, True} and any(g > 64 for g, _, _, _ in V.CONFIGS)
    # the scored Q's column rule (5 r + 32) % 36 gives neighbouring heads different columns: 5 n_q % 36 != 0 for every chunk
    assert all((5 * nq) % 36 for nq in V.N_Q if nq)


def test_helper_pieces_are_mla_probe_s_and_packing_inverts():
    assert V.SCORE_COLS is M.SCORE_COLS and V.SPLITS is D.SPLITS and V.violations is D.violations and V.restate is M.restate
    assert len({c_log2e(D.SCALE, dt) for dt in DTYPES}) == 1                              # one truth serves the three dtypes
    whole1, whole2 = M.latent_cache(lens=V.N_K, s_k=V.S_K), M.latent_cache(lens=[n for n in V.N_K for _ in range(2)], s_k=V.S_K)
    sc = torch.tensor(M.SCORE_COLS)
    for b, nk in enumerate(V.N_K):
        assert torch.equal(V.seq_cache(1, b), whole1[b:b + 1])                           # slices of mla_probe's own
        assert torch.equal(V.seq_cache(2, b), whole2[2 * b:2 * b + 2])
        assert (V.cache(2)[b, :, nk:][..., sc] == 8).all() and (V.cache(1)[b, :, nk:][..., sc] == 8).all()   # decoys behind N_K[b]
    assert not torch.equal(V.cache(2)[3, 0], V.cache(2)[3, 1])                            # each KV head its own key offset
    for g, h_kv, n_q in ((5, 1, 17), (16, 2, 3), (40, 1, 70), (128, 1, 1), (1, 1, 64)):
        Q = V.seq_queries(g, n_q, False, h_kv)
        assert torch.equal(Q[:1], M.queries(g, n_q, B=3)[1:2]) and Q.shape == (h_kv, 1, g * n_q, 576)
        P = V.pack(Q, g, n_q)
        assert P.shape == (n_q, g * h_kv, 576) and torch.equal(V.group(P, g), Q)
        for hk in range(h_kv):                                                           # both orderings, spelled out
            for pos, hg in ((0, 0), (n_q - 1, g - 1), (n_q // 2, g // 3)):
                assert torch.equal(P[pos, hk * g + hg], Q[hk, 0, hg * n_q + pos])
                assert V.kernel_rows(g, n_q)[pos * g + hg] == hg * n_q + pos and V.probe_rows(g, n_q)[hg * n_q + pos] == pos * g + hg
        for name in ("head_major", "rotated_tile", "plus32_packed"):
            src = V.row_source(name, g, n_q, 3)
            assert src.min() >= 0 and src.max() < g * n_q
            if name == "head_major" or (name == "rotated_tile" and (g * n_q) % 64 == 0):
                assert sorted(src.tolist()) == list(range(g * n_q))                       # a permutation (whole tiles)
    whole = M.decode_keep(5, 17, True, (64, 0), lens=V.N_K, s_k=V.S_K)
    assert torch.equal(V.seq_keep(5, 1, 5, True, (64, 0)), whole[5:6]) and V.N_Q[5] == 17
    assert V.packed_queries(16, 2, False).shape == (V.TOTAL, 32, 576)
    per = [(torch.full((1, 1, 5 * n, 512), float(b)), torch.full((1, 1, 5 * n, 1), float(b))) if n else None for b, n in enumerate(V.N_Q)]
    O, L = V.packed(per, 5)
    assert O.shape == (V.TOTAL, 5, 512) and L.shape == (5, V.TOTAL)
    assert all((O[V.CU[b]:V.CU[b + 1]] == b).all() and (L[:, V.CU[b]:V.CU[b + 1]] == b).all() for b in range(V.B))
    # the restatement at several counts is mla_probe.restate at each
    g, h_kv, b = 16, 2, 5
    Q, KV, keep = V.seq_queries(g, V.N_Q[b], False, h_kv), V.seq_cache(h_kv, b), V.seq_keep(g, h_kv, b, True, (64, 0))
    for uniform, dt in ((False, BF16), (True, F32)):
        Q = V.seq_queries(g, V.N_Q[b], uniform, h_kv)
        for n, (O, L) in V.seq_restate(g, h_kv, b, True, (64, 0), uniform, dt, (1, 3)).items():
            O1, L1 = M.restate(Q, KV, M.value_of(KV), keep, [V.N_K[b]] * h_kv, n, dt)
            assert torch.equal(O, O1) and torch.equal(L, L1)
        O1, L1 = M.mla_truth(Q, KV, keep, dt)
        O, L = V.seq_truth(g, h_kv, b, True, (64, 0), uniform, dt)
        assert torch.equal(O, O1) and torch.equal(L, L1)


def test_num_splits_0_resolves_to_one_split_and_to_several():
    auto = {}
    for g, h_kv, _, _ in V.CONFIGS:
        auto[(g, h_kv)] = _auto(g, h_kv, BF16)
        assert auto[(g, h_kv)] == V.split_formula(g, h_kv) == _formula(V.B, g * h_kv, h_kv, V.TOTAL, V.MAX_Q, V.S_K) == _auto(g, h_kv, F16)
    print("num_splits = 0 resolves to", auto)
    assert any(n > 1 for n in auto.values()) and any(n == 1 for n in auto.values())


@functools.lru_cache(maxsize=None)
def truths(k, uniform):
    g, h_kv, causal, window = V.CONFIGS[k]
    return V.ragged_truth(g, h_kv, causal, window, uniform, F32)


@pytest.mark.parametrize("k", range(len(V.CONFIGS)))
def test_unplanted_restatement_breaks_no_bar(k):
    g, h_kv, causal, window = V.CONFIGS[k]
    bad, worst_o, worst_l = [], 0.0, 0.0
    for uniform in (False, True):
        ref = truths(k, uniform)
        for dt in DTYPES:
            counts = sorted(set(V.SPLITS[1:]) | {_auto(g, h_kv, dt)})
            for b in SEQS:
                for n, (O, L) in V.seq_restate(g, h_kv, b, causal, window, uniform, dt, counts).items():
                    assert O.shape == ref[b][0].shape and O.shape[-1] == 512
                    v = V.violations(O, L, *ref[b], dt, n > 1)
                    if v:
                        bad.append((uniform, name_of(dt), b, n, v))
                    if dt == F32 and n > 1:
                        eo, el = D.fp32_ulp_error(O, L, *ref[b])
                        worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
    print(f"{V.CONFIGS[k]}: the restatement's worst float32 error over its split counts: {worst_o:.2f} fp32 ulps on O, {worst_l:.2f} on L")
    assert not bad, (V.CONFIGS[k], bad[:10])
    # the oracle's rule -- four times the reference's own measured error, up to a power of two -- on THIS measurement gives no wider
    # bar than the one in use (recorded: V.MEASURED_FP32_ULPS, inside the oracle's SPLIT_MEASURED)
    assert 4 * max(worst_o, worst_l) <= D.SPLIT_FP32_ULPS and V.MEASURED_FP32_ULPS <= D.SPLIT_MEASURED, (worst_o, worst_l)


def _first_row(O, L, O_ref, L_ref, dt, g, n_q):
    """(KV head, position, head of the group, what) of the first element of the kernel's order that breaks an unsplit bar"""
    nan, inf, nonzero, eo, el = _bars(O, L, O_ref, L_ref, dt)
    hit = (nan | inf | nonzero.any(-1, keepdim=True) | (eo > 1).any(-1, keepdim=True) | (el > 1))[:, 0, :, 0]   # (H_kv, R)
    hk, r = (int(x) for x in torch.nonzero(hit[:, V.kernel_rows(g, n_q)])[0])
    r = int(V.kernel_rows(g, n_q)[r])
    what = "nan" if nan[hk, 0, r].any() else "empty row" if inf[hk, 0, r].any() else \
        f"O != 0 in column {int(torch.nonzero(nonzero[hk, 0, r])[0])}" if nonzero[hk, 0, r].any() else \
        f"O off by {eo[hk, 0, r].max().item():.3g} ulps" if (eo[hk, 0, r] > 1).any() else f"L off by {el[hk, 0, r].max().item():.3g} ulps"
    return f"KV head {hk}, position {r % n_q}, head {r // n_q}: {what}"


@functools.lru_cache(maxsize=None)
def clean(k, uniform, b, dt):
    """the un-planted restatement of sequence b at one split"""
    g, h_kv, causal, window = V.CONFIGS[k]
    return V.seq_restate(g, h_kv, b, causal, window, uniform, dt, (1,))[1]


@functools.lru_cache(maxsize=None)
def proof(k):
    """every plant on configuration k -> ({plant: sequences it changes}, misses, {plant: one row the bars catch it in})"""
    g, h_kv, causal, window = V.CONFIGS[k]
    changed_in, misses, example = {}, [], {}
    for name in V.PLANTS:
        changed, caught = set(), {dt: set() for dt in DTYPES}
        for uniform in (False, True):
            ref = truths(k, uniform)
            for b in SEQS:
                if all(b in caught[dt] for dt in DTYPES):
                    continue                                                             # (the scored probe saw it in every dtype)
                stored = name in V.OUTPUT_PLANTS                                         # (the un-planted result, rows or columns moved)
                O_t, L_t = V.planted(name, g, h_kv, b, causal, window, uniform,
                                     (lambda *_: ref[b]) if stored else lambda q, kk, v, kp: M.truth(q, kk, v, kp, F32))
                if torch.equal(O_t, ref[b][0]) and torch.equal(L_t, ref[b][1]):
                    continue
                changed.add(b)
                for dt in DTYPES:
                    if b in caught[dt]:
                        continue
                    O_p, L_p = V.planted(name, g, h_kv, b, causal, window, uniform, (lambda *_: clean(k, uniform, b, dt)) if stored else
                                         lambda q, kk, v, kp: M.restate(q, kk, v, kp, [V.N_K[b]] * h_kv, 1, dt))
                    if V.violations(O_p, L_p, *ref[b], dt, dt == F32):                   # float32: the split bar, the wider of its two
                        caught[dt].add(b)
                        if name not in example and dt == BF16:
                            example[name] = (f"sequence {b} (n_q {V.N_Q[b]}, N_k {V.N_K[b]}), {'uniform' if uniform else 'scored'} probe, "
                                             + _first_row(O_p, L_p, *ref[b], dt, g, V.N_Q[b]))
        changed_in[name] = sorted(changed)
        misses += [(V.CONFIGS[k], name, name_of(dt), b, V.N_Q[b], V.N_K[b]) for dt in DTYPES for b in sorted(changed - caught[dt])]
    return changed_in, misses, example


@pytest.mark.parametrize("k", range(len(V.CONFIGS)))
def test_every_plant_breaks_a_bar_in_every_sequence_it_changes(k):
    """The planted restatement against the truth, each sequence judged on its own.  A plant changes a sequence where the fp64 truth
    of the planted computation differs from the un-planted truth; the scored probe must see it there, or the uniform one, in bf16,
    f16 and f32.  Nothing is left out."""
    changed_in, misses, example = proof(k)
    print(V.CONFIGS[k], {p: len(s) for p, s in changed_in.items()})
    for p, e in example.items():
        print(f"  {p}: {e}")
    assert not misses, misses[:20]


def test_every_plant_is_a_real_error_on_the_grid():
    """per plant, in how many (configuration, sequence) pairs it changed anything: above zero, and seen in all of them"""
    total = {p: 0 for p in V.PLANTS}
    missed = {p: 0 for p in V.PLANTS}
    for k in range(len(V.CONFIGS)):
        changed_in, misses, _ = proof(k)
        for p, s in changed_in.items():
            total[p] += len(s)
        for m in misses:
            missed[m[1]] += 1
    pairs = len(V.CONFIGS) * len(SEQS)
    for p in V.PLANTS:
        print(f"{p}: changed {total[p]} of {pairs} (configuration, sequence) pairs, " + ("seen in all" if not missed[p] else f"MISSED {missed[p]} times"))
    assert all(n > 0 for n in total.values()), total
    assert not any(missed.values()), missed
