"""CPU proof that oracle/fa2_decode_probe.py -- the exact-arithmetic probe tests/test_decode_probe_gpu.py runs through every
KV-cache decode form -- sees what it must, on every case of the GPU grid and for every sequence length of it on its own:

  * the inputs are exact in every dtype they are used in (fp8 caches under their descales included), scores are integers in [0, 8];
  * every planted decode error (a stale row leaking in, a 64-key tile or the last partial tile not read, top-left alignment, a
    neighbour's length, two V tiles exchanged, the KV head taken modulo H_kv, the rows of a KV group mixed up, a descale dropped
    or the two swapped) breaks a bar on the scored or on the uniform probe (the GPU test runs both), for every I/O dtype and
    head size, in every sequence the plant changes;
  * the fp32 restatement of the split kernels and the combine launch (emulate_split) passes the bars for every case and split
    count, and its own error is what the float32 / float64 split bar was derived from;
  * the old bar of tests/test_decode_gpu.py (O_TOL[bf16] = 5e-2) lets two exchanged V tiles through at every length.
"""
import functools
import math

import pytest
import torch

from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_bwd_arith as A
from oracle import fa2_decode_probe as D

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
B = len(D.LENS)


@functools.lru_cache(maxsize=None)
def cache(d):
    return D.probe_cache(d)


def test_probe_inputs_are_exact_and_scores_are_small_integers():
    for d in (40, 64, 128):
        K, V = cache(d)
        assert K.min() == 0 and K.max() == 8 and torch.equal(K, K.round())
        assert torch.equal(V.sum(-1), torch.full_like(V.sum(-1), 2.0)) and V.max() == 1         # two ones per key
        for dt in (F16, BF16, F32, F64):
            assert torch.equal(K.to(dt).double(), K) and torch.equal(V.to(dt).double(), V)
        for fmt in D.F8:
            K8, V8 = D.fp8_cache(K, V, fmt)
            assert K8.dtype == fmt and torch.equal(K8.double() * D.K_DESCALE, K) and torch.equal(V8.double() * D.V_DESCALE, V)
            assert A.c_log2e(D.SCALE, BF16) * D.K_DESCALE == 2.0
        assert not torch.equal(torch.tensor(9.0).to(torch.float8_e5m2).double(), torch.tensor(9.0).double())    # (why mod 9)
        for g, n_q, _, _ in D.CONFIGS + D.VALU_CONFIGS:
            for uniform in (False, True):
                Q = D.probe_queries(g, n_q, d, uniform)
                S = Q @ K.transpose(-1, -2)
                assert S.min() == 0 and S.max() == (0 if uniform else 8) and torch.equal(S, S.round())
                assert torch.equal(Q.to(BF16).double(), Q)
        # the sequences and the KV heads differ, the decoys hold the largest score and V rows of their own
        assert not torch.equal(K[3, 0, :30], K[3, 1, :30]) and not torch.equal(V[3, 0, :30], V[4, 0, :30])
        for b, nk in enumerate(D.LENS):
            assert (K[b, :, nk:] == 8).all() and (V[b, :, nk:].sum(-1) == 2).all()
    assert A.c_log2e(D.SCALE, F32) == 1.0


def test_split_rule_is_the_header_s():
    """fa2_decode_split (csrc/fa2_decode.h): c = ceil(N_k / num_splits) rounded up to 64"""
    for n, s, c in ((0, 4, 0), (1, 128, 64), (64, 1, 64), (65, 2, 64), (129, 2, 128), (1000, 3, 384), (2500, 7, 384),
                    (2500, 16, 192), (2500, 128, 64), (4097, 16, 320)):
        assert D.split_chunk(n, s) == c
        assert c == ((n + s - 1) // s + 63) & ~63


def _auto_splits(g, n_q, d, dtype):
    return _lib.kvcache_num_splits(B, g * D.H_KV, D.H_KV, n_q, D.S_K, d, convert_triton_dtype(dtype))


def _planted(g, n_q, causal, window, d, uniform, dtype, fp8):
    """name -> (O, L, changed): the fp64 truth of each planted error in the (B, H_kv, R, ...) layout and the sequences it must be
    seen in (where it changes what the kernel reads or writes; the row mix-ups: where the issue requires them, N_k >= 9 and no
    mask)"""
    K, V = cache(d)
    Q = D.probe_queries(g, n_q, d, uniform)
    keep = D.decode_keep(g, n_q, causal, window)
    ref = D.truth(Q, K, V, keep, dtype)
    visible = keep.any(-1).any(-1).view(B)
    out = {}
    for p in D.KEEP_PLANTS:
        kb = D.decode_keep(g, n_q, causal, window, plant=p)
        out[p] = D.truth(Q, K, V, kb, dtype) + ((kb != keep).any(-1).any(-1).view(B),)
    Vs = D.v_tile_swap(V)
    seen_keys = keep.any(-2).view(B, 1, -1)                                       # keys some row of the sequence sees
    out["v_tile_swap"] = D.truth(Q, K, Vs, keep, dtype) + (((Vs != V).any(-1) & seen_keys).any(-1).any(-1),)
    moved = bool((torch.arange(g * D.H_KV) % D.H_KV != torch.arange(g * D.H_KV) // g).any())
    out["kv_head_mod"] = D.kv_head_mod_truth(Q, K, V, keep, dtype, g, n_q) + (visible & moved,)
    plain = not causal and window is None
    long = torch.tensor([nk >= 9 for nk in D.LENS])
    for p in D.ROW_PLANTS:
        perm = D.row_permutation(p, g, n_q)
        moved = not torch.equal(perm, torch.arange(g * n_q))
        out[p] = (ref[0][:, :, perm], ref[1][:, :, perm], long & (plain and moved))
    if fp8:
        for p in D.FP8_PLANTS:
            out[p] = D.truth(Q, *D.fp8_plant(p, K, V), keep, dtype) + (visible,)
    return ref, out


def _caught(ref, planted, dtype):
    """{(plant, b)} of the required (plant, sequence) pairs that break a bar in `dtype`, each sequence judged on its own -- for
    float32 / float64 both the one-split and the wider split bar, since every configuration runs under both"""
    O_ref, L_ref = ref
    hit = set()
    for name, (O_b, L_b, changed) in planted.items():
        O_c, L_c = O_b.to(dtype), L_b.to(dtype)
        seen = changed.clone()
        for split in ((False, True) if dtype in (F32, F64) else (False,)):
            seen &= D.violated(O_c, L_c, O_ref, L_ref, dtype, split)
        hit |= {(name, b) for b in torch.nonzero(seen).flatten().tolist()}
    return hit


def test_per_sequence_verdict_is_violations_of_the_slice():
    K, V = cache(64)
    g, n_q, causal, window = D.CONFIGS[2]
    Q = D.probe_queries(g, n_q, 64)
    O_ref, L_ref = D.truth(Q, K, V, D.decode_keep(g, n_q, causal, window), F32)
    for plant in ("drop_tile", "top_left", None):
        O, L = D.truth(Q, K, V, D.decode_keep(g, n_q, causal, window, plant=plant), F32)
        O[3, 0, 0, 0] = math.nan
        L[5, 1, 2, 0] = math.inf
        for dt in (BF16, F32, F64):
            for split in (False, True):
                got = D.violated(O.to(dt), L.to(dt), O_ref, L_ref, dt, split)
                want = [bool(D.violations(O[b:b + 1].to(dt), L[b:b + 1].to(dt), O_ref[b:b + 1], L_ref[b:b + 1], dt, split))
                        for b in range(B)]
                assert got.tolist() == want and (plant is None) == (sum(want) == 2)


def _prove(d, dtypes, cfgs, fp8=False):
    """-> (table, misses).  A plant must break a bar on the scored or on the uniform probe: the uniform probe is evaluated where
    the scored one let something through (and for the first configuration, to keep it exercised)."""
    table, misses = {}, []
    for k, (g, n_q, causal, window) in enumerate(cfgs):
        for rep in ({F16, BF16, F32} & set(dtypes), {F64} & set(dtypes)):       # (c = 1 and c = 1 + 2.7e-9: one truth each)
            if not rep:
                continue
            order = sorted(rep, key=str)
            scored = _planted(g, n_q, causal, window, d, False, order[0], fp8)
            need, hits = {}, {}
            for dt in order:
                caught = _caught(*scored, dt)
                for name, (_, _, changed) in scored[1].items():
                    if name in D.FP8_PLANTS and dt not in (F16, BF16):        # (an fp8 cache goes with 16-bit Q)
                        continue
                    need[dt, name] = {(name, b) for b in torch.nonzero(changed).flatten().tolist()}
                    hits[dt, name] = [need[dt, name] & caught, set()]
            if k == 0 or any(need[key] - hits[key][0] for key in need):
                uniform = _planted(g, n_q, causal, window, d, True, order[0], fp8)
                for dt in order:
                    caught = _caught(*uniform, dt)
                    for key in need:
                        if key[0] == dt:
                            hits[key][1] = need[key] & caught
            for (dt, name), want in need.items():
                row = table.setdefault(name, [0, 0, 0, 0])
                missed = want - hits[dt, name][0] - hits[dt, name][1]
                row[0] += len(want)
                row[1] += len(hits[dt, name][0])
                row[2] += len(hits[dt, name][1])
                row[3] += len(missed)
                misses += [((g, n_q, causal, window), str(dt)[6:], name, D.LENS[b]) for _, b in sorted(missed)]
    print(f"d {d} {[str(t)[6:] for t in dtypes]}: plant, (sequence, dtype) pairs required / seen by the scored probe / by the "
          f"uniform probe where it was asked / missed by both")
    for name, row in table.items():
        print(f"  {name:20s} {row[0]:5d} {row[1]:5d} {row[2]:5d} {row[3]:5d}")
    return table, misses


@pytest.mark.parametrize("d", [64, 128])
def test_grid_plants_break_a_bar_f16_bf16_f32_and_fp8_cache(d):
    """c = 1: the 16-bit dtypes (with the fp8 cache's descale plants) and float32; the VALU form's cases (80 rows, three 16-row
    tiles) included"""
    table, misses = _prove(d, (F16, BF16, F32), D.CONFIGS + D.VALU_CONFIGS, fp8=True)
    assert not misses, misses[:20]
    for name in D.KEEP_PLANTS + D.INPUT_PLANTS + D.ROW_PLANTS + D.FP8_PLANTS:
        assert table[name][0] > 0, name               # every plant is a real error somewhere on the grid


@pytest.mark.parametrize("d,dtypes", [(40, (F32, F64)), (64, (F64,)), (128, (F64,))])
def test_grid_plants_break_a_bar_f64_and_the_padded_head_size(d, dtypes):
    """float64 I/O (c = 1 + 2.7e-9); d = 40 (w = 20) is the padded head size the GPU test runs float32 and float64 at"""
    table, misses = _prove(d, dtypes, D.CONFIGS + D.VALU_CONFIGS)
    assert not misses, misses[:20]
    for name in D.KEEP_PLANTS + D.INPUT_PLANTS + D.ROW_PLANTS:
        assert table[name][0] > 0, name


@pytest.mark.parametrize("d,dtypes", [(128, (F16, BF16)), (64, (F16, BF16))])
def test_emulate_split_passes_the_bars_16_bit(d, dtypes):
    """every case under every split count of the grid, what num_splits = 0 resolves to included"""
    K, V = cache(d)
    bad = []
    for g, n_q, causal, window in D.CONFIGS + D.VALU_CONFIGS:
        keep = D.decode_keep(g, n_q, causal, window)
        for uniform in (False, True):
            Q = D.probe_queries(g, n_q, d, uniform)
            for dt in dtypes:
                ref = D.truth(Q, K, V, keep, dt)
                counts = tuple(sorted(set(D.SPLITS[1:]) | {_auto_splits(g, n_q, d, dt)}))
                for n, (O, L) in D.emulate_splits(Q, K, V, keep, D.LENS, counts, dt).items():
                    v = D.violations(O, L, *ref, dt, n > 1)
                    if v:
                        bad.append(((g, n_q, causal, window), uniform, str(dt)[6:], n, v))
    assert not bad, bad[:10]


def test_emulate_split_passes_the_bars_f32_f64_and_the_split_bar_is_four_times_its_error():
    """d 64 and 40, as the GPU test runs them"""
    worst_o, worst_l, bad = D.measure_split_error(_auto_splits)
    assert not bad, bad[:10]
    print(f"emulate_split against the fp64 truth, f32 / f64 I/O, the whole grid: O {worst_o:.2f}, L {worst_l:.2f} fp32 ulps; "
          f"recorded {D.SPLIT_MEASURED}, bar {D.SPLIT_FP32_ULPS}")
    assert 1.5 < max(worst_o, worst_l) <= D.SPLIT_MEASURED * 1.05          # (libm differences between hosts)
    assert D.SPLIT_FP32_ULPS == 2.0 ** math.ceil(math.log2(4 * D.SPLIT_MEASURED))


def test_split_emulation_merges_what_the_unsplit_one_computes():
    """16-bit I/O: the probe's arithmetic is exact up to the normalisation, so every split count gives the same bits or the
    neighbouring ulp"""
    K, V = cache(64)
    g, n_q, causal, window = D.CONFIGS[0]
    keep = D.decode_keep(g, n_q, causal, window)
    Q = D.probe_queries(g, n_q, 64)
    O1, L1 = D.emulate_split(Q, K, V, keep, D.LENS, 1, BF16)
    for n in (2, 7, 128):
        O, L = D.emulate_split(Q, K, V, keep, D.LENS, n, BF16)
        assert ((O.double() - O1.double()).abs() <= A.ulp(O1.double(), BF16)).all()
        assert torch.equal(torch.isinf(L), torch.isinf(L1)) and (O[0] == 0).all() and torch.isinf(L[0]).all()   # N_k = 0


def test_truth_and_emulation_on_the_visible_extent_are_those_over_the_whole_capacity():
    """by_extent only leaves out keys no row sees: the same bits (c = 1: every sum is exact)"""
    from oracle import fa2_mask_probe as P
    K, V = cache(64)
    for g, n_q, causal, window in (D.CONFIGS[0], D.CONFIGS[2], D.CONFIGS[7]):
        keep = D.decode_keep(g, n_q, causal, window)
        Q = D.probe_queries(g, n_q, 64)
        for a, b in zip(D.truth(Q, K, V, keep, F32), P.truth(Q, K, V, keep, F32)):
            assert torch.equal(a, b)
        for dt in (BF16, F32):
            whole = D._emulate_splits(Q, K, V, keep, D.LENS, (1, 3, 128), dt)
            for i, n in enumerate((1, 3, 128)):
                O, L = D.emulate_split(Q, K, V, keep, D.LENS, n, dt)
                assert torch.equal(O, whole[2 * i]) and torch.equal(L, whole[2 * i + 1]), (n, dt)


def test_empty_rows_are_held_exactly():
    g, n_q, causal, window = 2, 3, True, (0, 0)
    K, V = cache(64)
    keep = D.decode_keep(g, n_q, causal, window)
    Q = D.probe_queries(g, n_q, 64)
    O_ref, L_ref = D.truth(Q, K, V, keep, BF16)
    # N_k = 0: every row; N_k = 1 under N_q = 3: the first two rows of each head
    assert torch.isinf(L_ref[0]).all() and torch.isinf(L_ref[1, :, [0, 1, 3, 4]]).all() and torch.isfinite(L_ref[1, :, [2, 5]]).all()
    for n in (1, 3):
        O, L = D.emulate_split(Q, K, V, keep, D.LENS, n, BF16)
        assert not D.violations(O, L, O_ref, L_ref, BF16, n > 1)
        bad = L.clone()
        bad[0, 0, 0] = 0.0
        assert D.violations(O, bad, O_ref, L_ref, BF16, n > 1)
        bad = O.clone()
        bad[0, 0, 0, 0] = 2.0 ** -40
        assert D.violations(bad, L, O_ref, L_ref, BF16, n > 1)


# ----------------------------------------------------------------------------- the old bar
OLD_LENS = [0, 1, 63, 64, 65, 1000, 4097, 4200]                # tests/test_decode_gpu.py: LENS, S_K = 4200


def _old_recipe(g, n_q, d, dtype, h_kv=2, s_k=4200):
    """tests/test_decode_gpu.py's make(): N(0, 1/4) from a CPU generator seeded with 7 d + g + N_q, in the (B, H_kv, R, d) layout"""
    gen = torch.Generator().manual_seed(7 * d + g + n_q)
    Q = (torch.randn(len(OLD_LENS), g * h_kv, n_q, d, generator=gen) * 0.5).to(dtype)
    K = (torch.randn(len(OLD_LENS), h_kv, s_k, d, generator=gen) * 0.5).to(dtype)
    V = (torch.randn(len(OLD_LENS), h_kv, s_k, d, generator=gen) * 0.5).to(dtype)
    return D.to_groups(Q, g, n_q), K, V


def test_old_o_tol_bar_misses_exchanged_v_tiles_at_every_length():
    """g 4, N_q 1, no mask, d 128, bf16, scale 1 / sqrt(d) -- CONFIGS[0] of tests/test_decode_gpu.py: V of the last two full 64-key
    tiles of every sequence exchanged moves O by less than O_TOL[bf16] = 5e-2 at every length that has two tiles (L does not
    depend on V), where the probe's one-ulp bar sees it at every length of its own grid."""
    g, n_q, d = 4, 1, 128
    Q, K, V = _old_recipe(g, n_q, d, BF16)
    keep = D.decode_keep(g, n_q, False, None, lens=OLD_LENS, s_k=4200)
    O, L = D.truth(Q, K, V, keep, BF16, scale=1 / math.sqrt(d))
    O_b, L_b = D.truth(Q, K, D.v_tile_swap(V, OLD_LENS, full_tiles=True), keep, BF16, scale=1 / math.sqrt(d))
    assert torch.equal(L, L_b)
    for b, nk in enumerate(OLD_LENS):
        err = (O_b[b] - O[b]).abs().max().item()
        print(f"N_k {nk}: max |O swapped - O| = {err:.4f}")
        assert (err > 1e-3) == (nk >= 128) and err <= 5e-2
    # the same plant on the probe's inputs, at the lengths of its grid that have two full tiles
    Kp, Vp = cache(d)
    keep = D.decode_keep(g, n_q, False, None)
    Qp = D.probe_queries(g, n_q, d)
    O_r, L_r = D.truth(Qp, Kp, Vp, keep, BF16)
    O_p, L_p = D.truth(Qp, Kp, D.v_tile_swap(Vp, full_tiles=True), keep, BF16)
    for b, nk in enumerate(D.LENS):
        s = slice(b, b + 1)
        assert bool(D.violations(O_p[s].to(BF16), L_p[s].to(BF16), O_r[s], L_r[s], BF16, False)) == (nk >= 128), nk
