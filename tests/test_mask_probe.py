"""CPU proof that oracle/fa2_mask_probe.py -- the exact-arithmetic probe tests/test_mask_probe_gpu.py runs through every
windowed and varlen forward -- sees a band that is off by one key, on every case of the GPU grid:

  * c = fp32(scale log2 e) is exactly 1.0 at the probe's scale (fp64 I/O: 1 + 2.7e-9, so fp64 keeps the 1e-6 bar);
  * every planted mask error (an edge one key out, the band shifted by one, top-left varlen alignment, one row's band from
    the neighbouring sequence) moves at least one element past the bars, for every I/O dtype and head size the grid runs;
  * a valid fp32 implementation (P rounded to the I/O dtype before P V, fp32 sums) passes them;
  * the old bar of tests/test_window_gpu.py (O_TOL[bf16] = 5e-2) misses the one-key leak at wide windows.
"""
import math

import pytest
import torch

from oracle import fa2_bwd_arith as A
from oracle import fa2_mask_probe as P

F8 = (torch.float8_e4m3fn, torch.float8_e5m2)
DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def test_probe_scale_gives_c_exactly_one():
    for dt in (torch.float16, torch.bfloat16, torch.float32) + F8:
        assert A.c_log2e(P.SCALE, dt) == 1.0
    c64 = A.c_log2e(P.SCALE, torch.float64)
    assert c64 != 1.0 and abs(c64 - 1.0) < 3e-9


def test_probe_inputs_are_exact_and_scores_small():
    for dt in DTYPES + F8:
        Q, K, V = P.dense_inputs(2, 3, 130, 64, dt)
        for t in (Q, K, V):
            assert t.dtype == dt
        Qd, Kd, Vd = P.dense_inputs(2, 3, 130, 64, torch.float64)
        assert torch.equal(Q.double(), Qd) and torch.equal(K.double(), Kd) and torch.equal(V.double(), Vd)
    S = Qd @ Kd.transpose(-1, -2)
    assert S.min() == 0 and S.max() == 8 and torch.equal(S, S.round())
    assert torch.equal(Vd.sum(-1), torch.full_like(Vd.sum(-1), 2.0))          # two ones per key
    assert not torch.equal(Kd[0, 0], Kd[0, 1]) and not torch.equal(Vd[0, 0], Vd[1, 2])   # heads differ


def _dtypes(window, causal, d):
    return DTYPES + (F8 if P.fp8_applies(window, causal, d) else ())


def _prove(Q, K, V, keep, planted, dtypes, what, emulate=True):
    """the planted masks fail the bars for every dtype; the fp32 emulation of the true mask passes them"""
    misses = []
    for dt in dtypes:
        q, k, v = (t.to(dt) for t in (Q, K, V))
        O_ref, L_ref = P.truth(q, k, v, keep, dt)
        if emulate:
            O_e, L_e = P.emulate(q, k, v, keep, dt)
            assert not P.violations(O_e, L_e, O_ref, L_ref, dt), (what, dt, P.violations(O_e, L_e, O_ref, L_ref, dt))
        for name, bad in planted.items():
            O_b, L_b = P.truth(q, k, v, bad, dt)
            if not P.violations(O_b.to(dt), L_b.to(dt), O_ref, L_ref, dt):
                misses.append((what, str(dt)[6:], name))
    return misses


def _planted_dense(N, window, causal):
    keep = P.dense_keep(N, causal, window)
    planted = {}
    for p in P.DENSE_PLANTS:
        bad = P.dense_keep(N, causal, window, plant=p)
        if not torch.equal(bad, keep):
            planted[p] = bad
    return keep, planted


@pytest.mark.parametrize("d", [64, 128])
def test_window_grid_plants_caught_and_fp32_passes(d):
    """(the GPU test runs both probes, the scored and the uniform one: a plant must fail one of them)"""
    misses, n_planted = [], 0
    for N, window, causal in P.window_cases():
        keep, planted = _planted_dense(N, window, causal)
        n_planted += len(planted)
        both = [set(_prove(*P.dense_inputs(1, 1, N, d, torch.float64, uniform), keep, planted, _dtypes(window, causal, d),
                           (N, window, causal))) for uniform in (False, True)]
        misses += sorted(both[0] & both[1], key=str)
    assert not misses, misses[:20]
    assert n_planted >= 1.5 * len(P.window_cases())      # (most cases have an edge to move)


@pytest.mark.parametrize("d", [64, 128])
def test_varlen_grid_plants_caught_and_fp32_passes(d):
    misses, n_planted = [], 0
    H = 2
    for lq, lk, window, causal in P.varlen_cases():
        keep, planted = _planted_varlen(lq, lk, window, causal)
        n_planted += len(planted)
        both = [set(_prove(*P.heads_first(*P.varlen_inputs(lq, lk, H, d, torch.float64, uniform)), keep, planted,
                           DTYPES, (str(lq), str(lk), window, causal))) for uniform in (False, True)]
        misses += sorted(both[0] & both[1], key=str)
    assert not misses, misses[:20]
    # every plant is a real error somewhere, top-left alignment and the neighbour's row included
    assert n_planted >= 4 * len(P.varlen_cases())


def _planted_varlen(lq, lk, window, causal):
    keep = P.varlen_keep(lq, lk, causal, window)
    planted = {}
    for p in P.PLANTS:
        bad = P.varlen_keep(lq, lk, causal, window, plant=p)
        if not torch.equal(bad, keep):
            planted[p] = bad
    return keep, planted


@pytest.mark.parametrize("d", [40, 64, 96, 128])
def test_layout_cases_plants_caught(d):
    """the cases of test_probe_strided_views_and_padded_head_sizes: dense at B 2 H 3 and the packed batch at H 3"""
    misses = []
    for N, window, causal in P.LAYOUT_CASES:
        keep, planted = _planted_dense(N, window, causal)
        both = [set(_prove(*P.dense_inputs(2, 3, N, d, torch.float64, uniform), keep, planted,
                           (torch.bfloat16, torch.float16), (N, window, causal))) for uniform in (False, True)]
        misses += sorted(both[0] & both[1], key=str)
    lq, lk, windows = P.LAYOUT_VARLEN
    for window, causal in windows:
        keep, planted = _planted_varlen(lq, lk, window, causal)
        assert planted
        misses += _prove(*P.heads_first(*P.varlen_inputs(lq, lk, 3, d, torch.float64)), keep, planted,
                         (torch.bfloat16, torch.float16), ("varlen", window, causal))
    assert not misses, misses


def test_fuzz_probe_cases_plants_caught():
    """the probe half of every case of tests/test_window_varlen_fuzz_gpu.py, at its own B, H, d and dtype"""
    misses, n_planted = [], 0
    for B, H, N, d, dtype, window, causal, _ in P.fuzz_window_cases():
        keep, planted = _planted_dense(N, window, causal)
        n_planted += len(planted)
        both = [set(_prove(*P.dense_inputs(B, H, N, d, torch.float64, uniform), keep, planted, (dtype,),
                           (B, H, N, d, window, causal))) for uniform in (False, True)]
        misses += sorted(both[0] & both[1], key=str)
    for lq, lk, H, d, dtype, window, causal, _ in P.fuzz_varlen_cases():
        keep, planted = _planted_varlen(lq, lk, window, causal)
        n_planted += len(planted)
        both = [set(_prove(*P.heads_first(*P.varlen_inputs(lq, lk, H, d, torch.float64, uniform)), keep, planted,
                           (dtype,), (str(lq), str(lk), H, d, window, causal))) for uniform in (False, True)]
        misses += sorted(both[0] & both[1], key=str)
    assert not misses, misses[:20]
    assert n_planted >= 96


def test_empty_rows_are_held_exactly():
    lq, lk = [40, 8, 0, 5], [8, 40, 6, 0]
    keep = P.varlen_keep(lq, lk, True, None)
    Q, K, V = P.heads_first(*P.varlen_inputs(lq, lk, 1, 64, torch.bfloat16))
    O_ref, L_ref = P.truth(Q, K, V, keep, torch.bfloat16)
    empty = torch.isinf(L_ref[0, :, 0])
    assert int(empty.sum()) == 32 + 5 and (O_ref[0, empty] == 0).all()
    O, L = P.emulate(Q, K, V, keep, torch.bfloat16)
    assert not P.violations(O, L, O_ref, L_ref, torch.bfloat16)
    bad = L.clone()
    bad[0, 0, 0] = 0.0                     # an empty row with a finite L
    assert P.violations(O, bad, O_ref, L_ref, torch.bfloat16)
    bad = O.clone()
    bad[0, 0, 0] = 2.0 ** -40              # ... or a nonzero O
    assert P.violations(bad, L, O_ref, L_ref, torch.bfloat16)


def test_uniform_probe_gives_log2_count():
    N, window = 200, (31, 17)
    keep = P.dense_keep(N, False, window)
    Q, K, V = P.dense_inputs(1, 1, N, 64, torch.bfloat16, uniform=True)
    _, L_ref = P.truth(Q, K, V, keep, torch.bfloat16)
    assert torch.allclose(L_ref[0, 0, :, 0], torch.log2(keep.sum(-1).double()), rtol=0, atol=1e-12)


# ----------------------------------------------------------------------------- the old bar
def _old_recipe(N, d, seed):
    """tests/test_window_gpu.py's inputs(): bf16 N(0, 1/4), CPU generator seeded with N + d"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(1, 2, N, d, generator=g) * 0.5).to(torch.bfloat16) for _ in range(3)]


@pytest.mark.parametrize("window", [(128, 128), (-1, 300)])
def test_old_o_tol_bar_misses_one_key_leak_at_wide_windows(window):
    """N 1000, d 128, bf16, the window tests' scale 1 / sqrt(d): one leaked key moves O by less than O_TOL[bf16] = 5e-2 on
    random inputs, where the probe's one-ulp bar sees it"""
    N, d = 1000, 128
    Q, K, V = _old_recipe(N, d, N + d)
    keep = P.dense_keep(N, False, window)
    O, _ = P.truth(Q, K, V, keep, torch.bfloat16, scale=1 / math.sqrt(d))
    plants = [p for p in ("right_plus_one", "left_minus_one") if window[0 if p[0] == "l" else 1] >= 0]
    for p in plants:
        O_b, _ = P.truth(Q, K, V, P.dense_keep(N, False, window, plant=p), torch.bfloat16, scale=1 / math.sqrt(d))
        err = (O_b - O).abs().max().item()
        print(f"{window} {p}: max |O leak - O| = {err:.4f}")
        assert 1e-3 < err <= 5e-2
        q, k, v = P.dense_inputs(1, 1, N, d, torch.bfloat16)
        pk = P.dense_keep(N, False, window, plant=p)
        O_r, L_r = P.truth(q, k, v, keep, torch.bfloat16)
        O_p, L_p = P.truth(q, k, v, pk, torch.bfloat16)
        assert P.violations(O_p.to(torch.bfloat16), L_p.to(torch.bfloat16), O_r, L_r, torch.bfloat16)
