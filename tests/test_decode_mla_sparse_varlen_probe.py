"""CPU proof that tests/mla_sparse_varlen_probe.py -- the exact-arithmetic probe tests/test_decode_mla_sparse_varlen_probe_gpu.py runs
through sparse MLA decode of packed queries (fa2_fwd_kvcache_mla_sparse_varlen) -- sees what it must:

  * the batch holds a leading empty sequence, two empty sequences in a row, a trailing one, a B that takes the owner search four steps
    deep, a token whose sequence has no key, three tokens over two keys, a sequence at full capacity, all lengths different; the lists
    hold distinct valid positions of the row's own sequence mixed with every kind of entry that is no key, one list has no valid entry
    although its sequence has keys, where topk > 64 one has all of them behind slot 64, and the two lists of a row differ;
  * the un-planted restatement (emulate_split over the slots of the gathered rows, one pseudo-sequence per (packed row, KV head))
    breaks no bar on any configuration, scored and uniform, in bf16, f16 and f32, at every split count of SPLITS and at what
    num_splits = 0 resolves to; its worst float32 error in fp32 ulps is measured and printed;
  * every planted error -- the ten of the packed layout and mla_sparse_probe's nine, per list -- breaks a bar in every (packed row,
    KV head) whose truth it changes, in every dtype, on the scored or on the uniform probe, judged row by row with the reference
    restatement alone; and every plant is a real error on some configuration.

Bars: oracle/fa2_decode_probe.violations -- 16-bit I/O one output ulp on O and L, exact zeros, exact empty rows at any num_splits;
float32 its 4 ulps unsplit and SPLIT_FP32_ULPS split."""
import functools

import pytest
import torch

import mla_probe as M
import mla_sparse_probe as S
import mla_sparse_varlen_probe as V
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = (BF16, F16, F32)
name_of = lambda dt: str(dt)[6:]


def _auto(H, h_kv, topk, dtype):
    return _lib.kvcache_mla_sparse_varlen_num_splits(V.TOTAL, H, h_kv, topk, 576, 512, convert_triton_dtype(dtype))


def owner_search(t, cu=V.CU, B=V.B):
    """fa2_varlen_owner's search, restated: the last b in [0, B) whose offset is <= t, and the number of steps it took"""
    lo, hi, steps = 0, B, 0
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        lo, hi = (mid, hi) if cu[mid] <= t else (lo, mid)
        steps += 1
    return lo, steps


def test_the_batch_holds_what_it_must():
    assert V.N_Q == [0, 1, 3, 0, 0, 2, 5, 1, 17, 4, 0] and V.N_K == [100, 0, 2, 64, 7, 65, 64, 2560, 1000, 300, 50]
    assert (V.S_K, V.B, V.TOTAL, V.MAX_Q) == (2560, 11, 33, 17) and V.CU == [0, 0, 1, 4, 4, 4, 6, 11, 12, 29, 33, 33]
    assert V.SPLITS == (0, 1, 3, 16, 128) and V.SPLITS is S.SPLITS and V.NO_KEY is S.NO_KEY
    assert V.violations is D.violations and V.violated is D.violated and V.restate is M.restate and V.mla_truth is M.mla_truth
    pairs = list(zip(V.N_Q, V.N_K))
    assert V.N_Q[0] == 0 and V.N_Q[-1] == 0                                               # a leading and a trailing empty sequence
    assert any(V.N_Q[b] == V.N_Q[b + 1] == 0 and V.N_Q[b + 2] > 0 for b in range(1, V.B - 2))   # two in a row, a row behind them
    assert any(nq == 1 and nk == 0 for nq, nk in pairs) and (3, 2) in pairs               # a token without a key; three over two keys
    assert any(nq and nk == V.S_K for nq, nk in pairs)                                    # a sequence at full capacity
    # the lengths of the sequences that own rows all differ, and each differs from both its neighbours' and from that of the first
    # sequence at its offset: a row given another sequence's length or rows shows
    owning = [b for b in range(V.B) if V.N_Q[b]]
    assert len({V.N_K[b] for b in owning}) == len(owning)
    assert all(V.N_K[b] != V.N_K[o] for b in owning for o in ((b + 1) % V.B, (b - 1) % V.B, V.first_of_equal_offsets(b)) if o != b)
    found = [owner_search(t) for t in range(V.TOTAL)]
    assert [b for b, _ in found] == V.OWNER and max(s for _, s in found) == 4             # the search is four steps deep
    assert all(V.CU[b] + i == t for t, (b, i) in enumerate(zip(V.OWNER, V.POS)))
    assert [V.first_of_equal_offsets(b) for b in range(V.B) if V.N_Q[b]] == [0, 2, 3, 6, 7, 8, 9]   # (of sequences 1, 2, 5, 6, 7, 8, 9)
    # the configurations: a quarter, a partial, one and two head tiles; every topk; two KV heads twice, once with g = 128
    assert {H // h_kv for H, h_kv, _ in V.CONFIGS} == {16, 40, 64, 128} and {c[2] for c in V.CONFIGS} == {1, 63, 64, 65, 200, 2048}
    assert sum(h_kv == 2 for _, h_kv, _ in V.CONFIGS) >= 2 and (256, 2) in {c[:2] for c in V.CONFIGS}
    for r in range(len(V.SPLITS)):
        assert [c[:3] for c in V.cases(r)] == V.CONFIGS
    assert all({V.cases(r)[k][3] for r in range(len(V.SPLITS))} == set(V.SPLITS) for k in range(len(V.CONFIGS)))
    # the cache is mla_varlen_probe.cache's rule: (b, h) is row set u = b H_kv + h, decoys behind N_K[b]
    whole = M.latent_cache(lens=[n for n in V.N_K for _ in range(2)], s_k=V.S_K)
    sc = torch.tensor(M.SCORE_COLS)
    for b, nk in enumerate(V.N_K):
        assert torch.equal(V.cache(2)[b], whole[2 * b:2 * b + 2, 0]) and (V.cache(2)[b, :, nk:][..., sc] == 8).all()
    # the queries: token i of sequence b, head hk g + hg, is row hg n_q(b) + i of mla_probe.queries(g, n_q(b))
    Q = V.packed_queries(16, 2)
    assert Q.shape == (V.TOTAL, 32, 576)
    for t in (0, 3, 12, 20, 32):
        b, i = V.OWNER[t], V.POS[t]
        for hg in (0, 5, 15):
            want = M.queries(16, V.N_Q[b], B=1)[0, 0, hg * V.N_Q[b] + i]
            assert torch.equal(Q[t, hg], want) and torch.equal(Q[t, 16 + hg], want)
    assert not V.packed_queries(16, 2, uniform=True).any()
    assert all((5 * nq) % 36 for nq in V.N_Q if nq)                                       # neighbouring heads score on different columns


def test_lists_hold_what_they_must():
    kinds = set()
    for H, h_kv, topk in V.CONFIGS:
        idx = V.lists(h_kv, topk)
        ok = V.valid(idx)
        assert idx.shape == (V.TOTAL, h_kv, topk) and idx.dtype == torch.int32 and idx.is_contiguous()
        assert not ok[V.EMPTY_T, 0].any() and V.N_K[V.OWNER[V.EMPTY_T]] > 0               # a list with none though its sequence has keys
        assert not ok[0].any() and V.N_K[V.OWNER[0]] == 0                                 # the token whose sequence has no key
        for t, b in enumerate(V.OWNER):
            nk = V.N_K[b]
            for hk in range(h_kv):
                j = idx[t, hk][ok[t, hk]]
                assert j.unique().numel() == j.numel() and (j >= 0).all() and (j < nk).all()   # distinct, of the row's own sequence
                kinds |= set(idx[t, hk][~ok[t, hk]].tolist()) - {nk}
                if (idx[t, hk] == nk).any():
                    kinds.add("nk")
            if h_kv == 2 and topk > 1:
                assert not torch.equal(idx[t, 0], idx[t, 1])                              # the two lists of a row differ
        if topk > 64:
            late = ok[V.LATE_T, 0]
            assert late[64:].any() and not late[:64].any()                                # all valid entries behind slot 64
            assert ok.reshape(-1, topk)[:, :64].any() and ok[V.CU[7]:].sum() > ok[V.CU[7]:].numel() // 4
        two = ok[V.CU[2]:V.CU[3]]                                                         # three tokens over two keys: almost all no key
        assert two.sum(-1).max() <= 2 and (topk == 1 or two.any())
    assert kinds >= {-1, "nk", V.S_K + 5, 2 ** 31 - 1, -2 ** 31}


def test_layouts_invert_and_the_gather_is_mla_sparse_probe_s():
    g, h_kv, topk = 16, 2, 200
    Q, K, keep = V.operands(g, h_kv, topk)
    P = V.TOTAL * h_kv
    assert Q.shape == (P, 1, g, 576) and K.shape == (P, 1, topk, 576) and keep.shape == (P, 1, g, topk)
    idx, ok = V.lists(h_kv, topk), V.valid(V.lists(h_kv, topk))
    assert torch.equal(keep[:, 0, 0], ok.reshape(P, topk))
    for t, hk, s in ((12, 0, 70), (12, 1, 3), (32, 1, 199), (5, 0, 0)):
        p = t * h_kv + hk
        j = int(idx[t, hk, s]) if ok[t, hk, s] else 0
        if ok[t, hk, s]:
            assert torch.equal(K[p, 0, s], V.cache(h_kv)[V.OWNER[t], hk, j])
        assert torch.equal(Q[p, 0], V.packed_queries(g, h_kv)[t, hk * g:(hk + 1) * g])
    O = torch.arange(P * g * 512, dtype=torch.float64).view(P, 1, g, 512)
    L = torch.arange(P * g, dtype=torch.float64).view(P, 1, g, 1)
    Oc, Lc = V.to_call(O, L, h_kv)
    assert Oc.shape == (V.TOTAL, h_kv * g, 512) and Lc.shape == (h_kv * g, V.TOTAL)
    assert torch.equal(Oc[7, g + 3], O[7 * h_kv + 1, 0, 3]) and Lc[g + 3, 7] == L[7 * h_kv + 1, 0, 3, 0]
    O2, L2 = V.from_call(Oc, Lc, h_kv)
    assert torch.equal(O2, O) and torch.equal(L2, L)
    H = h_kv * g
    Om, Lm = V.to_call(*V.moved("partials_head_major", O, L, h_kv), h_kv)
    for t, head in ((0, 0), (5, 3), (32, 31)):
        f = head * V.TOTAL + t
        assert torch.equal(Om[t, head], Oc[f // H, f % H]) and Lm[head, t] == Lc[f % H, f // H]
    Ol, Ll = V.to_call(*V.moved("l_transposed", O, L, h_kv), h_kv)
    assert torch.equal(Ol, Oc)
    for t, head in ((0, 0), (5, 3), (32, 31)):
        f = head * V.TOTAL + t
        assert Ll[head, t] == Lc[f % H, f // H]


@functools.lru_cache(maxsize=None)
def truths(k, uniform):
    """(Q, K, keep) and the fp64 truth of configuration k (c = 1 for the three dtypes alike: one truth serves them)"""
    H, h_kv, topk = V.CONFIGS[k]
    ops = V.operands(H // h_kv, h_kv, topk, uniform)
    return ops, V.truth(*ops, F32)


@pytest.mark.parametrize("k", range(len(V.CONFIGS)))
def test_unplanted_restatement_breaks_no_bar(k):
    H, h_kv, topk = V.CONFIGS[k]
    bad, worst_o, worst_l = [], 0.0, 0.0
    for uniform in (False, True):
        (Q, K, keep), ref = truths(k, uniform)
        for dt in DTYPES:
            for n in sorted(set(V.SPLITS[1:]) | {_auto(H, h_kv, topk, dt)}):
                O, L = V.restate_slots(Q, K, keep, n, dt)
                assert O.shape == (V.TOTAL * h_kv, 1, H // h_kv, 512)
                v = V.violations(O, L, *ref, dt, n > 1)
                if v:
                    bad.append((uniform, name_of(dt), n, v))
                if dt == F32 and n > 1:
                    eo, el = V.fp32_ulp_error(O, L, *ref)
                    worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
    print(f"{V.CONFIGS[k]}: the restatement's worst float32 error over its split counts: {worst_o:.2f} fp32 ulps on O, {worst_l:.2f} on L")
    assert not bad, (V.CONFIGS[k], bad[:10])
    assert max(worst_o, worst_l) <= V.MEASURED_FP32_ULPS <= D.SPLIT_MEASURED, (worst_o, worst_l)


def test_num_splits_0_resolves_to_one_split_and_to_several():
    auto = {cfg: _auto(*cfg, BF16) for cfg in V.CONFIGS}
    print("num_splits = 0 resolves to", auto)
    assert all(_auto(*cfg, F16) == n for cfg, n in auto.items())
    assert any(n > 1 for n in auto.values()) and any(n == 1 for n in auto.values())


@functools.lru_cache(maxsize=None)
def proof(k):
    """every plant on configuration k -> ({plant: number of (packed row, KV head) it changes, or None: cannot apply}, misses)"""
    H, h_kv, topk = V.CONFIGS[k]
    g, P = H // h_kv, V.TOTAL * h_kv
    changed_in, misses = {}, []
    for name in V.PLANTS:
        changed = torch.zeros(P, dtype=torch.bool)
        caught = {dt: torch.zeros(P, dtype=torch.bool) for dt in DTYPES}
        applies = False
        for uniform in (False, True):
            _, (O_ref, L_ref) = truths(k, uniform)
            got = V.planted_outputs(name, lambda q, kk, kp: V.truth(q, kk, kp, F32), g, h_kv, topk, uniform)
            if got is None:
                continue
            applies = True
            O_t, L_t = got
            ch = (O_t != O_ref).reshape(P, -1).any(-1) | (L_t != L_ref).reshape(P, -1).any(-1)
            if not ch.any():
                continue
            changed |= ch
            for dt in DTYPES:
                if not (ch & ~caught[dt]).any():
                    continue                                                              # (the scored probe saw them all)
                O_p, L_p = V.planted_outputs(name, lambda q, kk, kp: V.restate_slots(q, kk, kp, 1, dt), g, h_kv, topk, uniform)
                hit = V.violated(O_p, L_p, O_ref, L_ref, dt, False)
                if dt == F32:                                                             # every configuration runs split as well
                    hit &= V.violated(O_p, L_p, O_ref, L_ref, dt, True)
                caught[dt] |= ch & hit
        changed_in[name] = int(changed.sum()) if applies else None
        for dt in DTYPES:
            misses += [(V.CONFIGS[k], name, name_of(dt), p // h_kv, p % h_kv) for p in torch.nonzero(changed & ~caught[dt]).flatten().tolist()]
    return changed_in, misses


@pytest.mark.parametrize("k", range(len(V.CONFIGS)))
def test_every_plant_breaks_a_bar_in_every_row_and_kv_head_it_changes(k):
    """The planted restatement against the truth, each (packed row, KV head) judged on its own.  A plant changes one where the fp64
    truth of the planted computation differs from the un-planted truth; the scored probe must see it there, or the uniform one, in
    bf16, f16 and f32.  Nothing is left out."""
    H, h_kv, topk = V.CONFIGS[k]
    changed_in, misses = proof(k)
    print(V.CONFIGS[k], changed_in)
    assert not misses, misses[:20]
    # on this configuration every plant that can apply is a real error somewhere
    expect = set(V.PLANTS)
    if h_kv < 2:
        expect -= {"kv_head_0_list", "kv_head_other_cache"}
    if topk % 64 == 0:
        expect -= {"past_topk_read", "drop_last_partial"}
    if D.split_chunk(topk, 3) >= topk:
        expect -= {"boundary_twice", "boundary_skipped"}
    assert all(changed_in[p] is None for p in set(V.PLANTS) - expect)
    if topk == 1:
        expect -= {p for p in expect if not changed_in[p]}   # (33 lists of one slot: a plant may change none of them)
    assert all(changed_in[p] for p in expect), (V.CONFIGS[k], {p: changed_in[p] for p in expect if not changed_in[p]})


def test_every_plant_is_a_real_error_on_the_grid():
    """per plant, in how many (packed row, KV head) pairs of the whole grid it changed anything: above zero, and seen in all"""
    total = {p: 0 for p in V.PLANTS}
    missed = {p: 0 for p in V.PLANTS}
    for k in range(len(V.CONFIGS)):
        changed_in, misses = proof(k)
        for p, n in changed_in.items():
            total[p] += n or 0
        for m in misses:
            missed[m[1]] += 1
    pairs = sum(V.TOTAL * h_kv for _, h_kv, _ in V.CONFIGS)
    for p in V.PLANTS:
        print(f"{p}: changed {total[p]} of {pairs} (packed row, KV head) pairs, " + ("seen in all" if not missed[p] else f"MISSED {missed[p]} times"))
    assert all(n > 0 for n in total.values()), total
    assert not any(missed.values()), missed
