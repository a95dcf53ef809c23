"""CPU pins of oracle/fa2_bwd_arith.py -- the restatement of the backward kernels' arithmetic that
tests/test_bwd_elementwise.py holds every backward kernel to, element by element -- and proof that its bars see errors.

  * the restatement against the references already in the suite: oracle.grads_f64 (fp32), the bwd_* goldens (reference
    kernels and fp64 SDPA autograd, with the bars tests/test_bwd_parity.py applies to the kernels) and
    attention_backward_recompute (fp64);
  * the same arithmetic run in fp32 (what the kernels' precision allows) passes the bars;
  * errors planted in the restatement fail them, and the old max-norm bar (REL = 2.5e-2 for bf16) misses two of them.
"""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import fa2_bwd_arith as A
from oracle import fa2_oracle

REL = {torch.float16: 4e-3, torch.bfloat16: 2.5e-2}           # tests/test_bwd_parity.py
REL_ORACLE = {torch.float16: 2e-2, torch.bfloat16: 1.2e-1}


def stored_forward(Q, K, V, causal=False, scale=1.0):
    """O and L as the forward stores them: the fp64 values rounded once to the I/O dtype."""
    O, L = fa2_oracle.sdpa_f64(Q.double().numpy(), K.double().numpy(), V.double().numpy(), causal=causal, scale=scale)
    return torch.from_numpy(O).to(Q.dtype), torch.from_numpy(L).to(Q.dtype)


def rand4(shape, dtype, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn(*shape, generator=g) * spread).to(dtype) for _ in range(4))


def bf16(u16):
    return torch.from_numpy(u16.view(np.int16).copy()).view(torch.bfloat16)


# ----------------------------------------------------------------------------- pins
@pytest.mark.parametrize("kernel", A.KERNELS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape,scale", [((1, 2, 65, 64), 1.0), ((2, 1, 130, 128), 0.3), ((1, 1, 17, 16), 1 / 4)])
def test_fp32_restatement_matches_grads_f64(kernel, causal, shape, scale):
    Q, K, V, dO = rand4(shape, torch.float32, seed=shape[2] + int(causal))
    O, L = stored_forward(Q, K, V, causal, scale)
    got = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, bars=False)
    truth = fa2_oracle.grads_f64(Q.numpy(), K.numpy(), V.numpy(), dO.numpy(), causal=causal, scale=scale)
    for name, a, t in zip(("dQ", "dK", "dV"), got, truth):
        assert a.dtype == torch.float32
        assert np.abs(a.double().numpy() - t).max() <= 1e-5 * np.abs(t).max(), name


@pytest.mark.parametrize("kernel", A.KERNELS)
def test_goldens_fp32(kernel):
    for name in ("bwd_test_torch_f32_seed5", "bwd_c1_f32_seed11"):
        g = load_golden(name)
        Q, K, V, dO, O, L = (torch.from_numpy(g[k]) for k in ("Q", "K", "V", "dO", "O_ref", "L_ref"))
        got = A.restate(Q, K, V, O, L, dO, False, 1.0, kernel, bars=False)
        for k, a, atol in (("dQ", got[0], 9e-4), ("dK", got[1], 7e-4), ("dV", got[2], 7e-5)):
            assert torch.allclose(torch.from_numpy(g[f"{k}_sdpa"]), a, atol=atol, rtol=1e-5), (name, k)
            assert (a - torch.from_numpy(g[f"{k}_ref"])).abs().max() < 4e-4, (name, k)
    g = load_golden("bwd_c1_f32_causal_seed13")
    Q, K, V, dO = (torch.from_numpy(g[k]) for k in ("Q", "K", "V", "dO"))
    for causal, sfx in ((False, ""), (True, "_causal")):
        O, L = stored_forward(Q, K, V, causal)
        got = A.restate(Q, K, V, O, L, dO, causal, 1.0, kernel, bars=False)
        for k, a, atol in (("dQ", got[0], 9e-4), ("dK", got[1], 7e-4), ("dV", got[2], 7e-5)):
            assert torch.allclose(torch.from_numpy(g[f"{k}_sdpa{sfx}"]), a, atol=atol, rtol=1e-5), (causal, k)


@pytest.mark.parametrize("kernel", ["mfma16", "generic"])
def test_goldens_16bit(kernel):
    g = load_golden("bwd_c1_f16_seed12")        # the reference's own forward outputs (O_ref, L_ref in fp16)
    Q, K, V, dO, O, L = (torch.from_numpy(g[k]) for k in ("Q", "K", "V", "dO", "O_ref", "L_ref"))
    got = A.restate(Q, K, V, O, L, dO, False, 1.0, kernel, bars=False)
    for k, a in zip(("dQ", "dK", "dV"), got):
        truth = torch.from_numpy(g[f"{k}_sdpa"])
        assert a.dtype == torch.float16
        assert (a.float() - truth).abs().max() <= REL[torch.float16] * truth.abs().max(), k
        ref = torch.from_numpy(g[f"{k}_ref"]).float()
        assert (a.float() - ref).abs().max() <= REL_ORACLE[torch.float16] * truth.abs().max(), k
    g = load_golden("bwd_c1_bf16_seed14")
    Q, K, V, dO = (bf16(g[k]) for k in ("Q", "K", "V", "dO"))
    for causal, sfx in ((False, ""), (True, "_causal")):
        O, L = stored_forward(Q, K, V, causal)
        got = A.restate(Q, K, V, O, L, dO, causal, 1.0, kernel, bars=False)
        for k, a in zip(("dQ", "dK", "dV"), got):
            truth = torch.from_numpy(g[f"{k}_sdpa{sfx}"])
            assert (a.float() - truth).abs().max() <= REL[torch.bfloat16] * truth.abs().max(), (causal, k)


@pytest.mark.parametrize("causal", [False, True])
def test_fp64_matches_attention_backward_recompute(causal):
    from flash_attention_dlrs_amd.flash_attention_torch import attention_backward_recompute
    Q, K, V, dO = rand4((1, 2, 72, 32), torch.float64, seed=4)
    O, L = stored_forward(Q, K, V, causal, 0.7)
    got = A.restate(Q, K, V, O, L, dO, causal, 0.7, "generic", bars=False)
    want = attention_backward_recompute(Q, K, V, O, dO, L, causal=causal, scale=0.7)
    for a, w in zip(got, want):
        assert a.dtype == torch.float64 and (a - w).abs().max() <= 1e-12 * w.abs().max()


def test_rounding_points():
    """rnd is torch's RTNE conversion with subnormals kept; c is fp32(scale log2 e) formed in double"""
    x = torch.tensor([2.0 ** -24, 3 * 2.0 ** -26, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], dtype=torch.float64)
    assert A.rnd(x, torch.float16).tolist() == [2.0 ** -24, 2.0 ** -24, 1.0, 1 + 2.0 ** -9]
    assert A.rnd(x, torch.float32) is x
    assert A.c_log2e(0.3, torch.bfloat16) == float(np.float32(0.3 * math.log2(math.e)))
    assert A.c_log2e(0.3, torch.float64) == 0.3 * math.log2(math.e)
    assert A.ulp(torch.tensor([1.0, 0.75, 0.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -8, 2.0 ** -133]


# ----------------------------------------------------------------------------- the bars
# (shape, dtype, causal, scale, spread, kernel): shapes and distributions of tests/test_bwd_elementwise.py's matrix
BAR_CASES = [((1, 2, 512, 128), torch.bfloat16, True, 1.0, 1.0, "mfma16"),                  # N(0, 1) at scale 1 (the bench)
             ((1, 2, 257, 64), torch.bfloat16, True, 0.3, 0.5, "mfma16"),                   # ragged N, scale 0.3
             ((1, 2, 1000, 128), torch.float16, False, 1 / math.sqrt(128), 1.0, "mfma16"),
             ((1, 2, 129, 64), torch.float16, True, 0.3, 0.5, "generic"),
             ((1, 2, 255, 64), torch.float32, True, 0.3, 1.0, "mfma32")]


def _case(shape, dtype, causal, scale, spread):
    Q, K, V, dO = rand4(shape, dtype, seed=shape[2], spread=spread)
    O, L = stored_forward(Q, K, V, causal, scale)
    return Q, K, V, O, L, dO


@pytest.mark.parametrize("case", BAR_CASES, ids=lambda c: f"{c[5]}-{str(c[1])[6:]}-N{c[0][2]}-causal{int(c[2])}")
def test_fp32_arithmetic_passes_the_bars(case):
    """the restatement's arithmetic run in fp32 -- the kernels' precision, with another summation order and fp32 exp2 / Lc --
    is a valid implementation: it must pass the bars against the fp64 restatement"""
    shape, dtype, causal, scale, spread, kernel = case
    Q, K, V, O, L, dO = _case(shape, dtype, causal, scale, spread)
    ref = A.restate(Q, K, V, O, L, dO, causal, scale, kernel)
    emu = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, bars=False, acc=torch.float32)
    A.assert_close(emu[:3], ref, case)


def test_planted_errors_fail_the_bars():
    """each error planted in the restatement fails compare() against the clean restatement on at least one case of the
    matrix; the report names the case(s) that catch it"""
    caught = {p: [] for p in A.PLANTS}
    for case in BAR_CASES:
        shape, dtype, causal, scale, spread, kernel = case
        Q, K, V, O, L, dO = _case(shape, dtype, causal, scale, spread)
        ref = A.restate(Q, K, V, O, L, dO, causal, scale, kernel)
        for p in A.PLANTS:
            bad = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, plant=p, bars=False)
            rep = A.compare(bad[:3], ref)
            failed = [(n, round(s, 3), round(w, 1)) for n, s, w, ok in rep if not ok]
            if failed:
                caught[p].append((f"{kernel} {str(dtype)[6:]} N={shape[2]} causal={causal} scale={scale:.3g}", failed))
    for p, by in caught.items():
        print(f"{p}: caught by {by}")
    assert all(caught.values()), {p: by for p, by in caught.items() if not by}
    # the case that carries all of them: bf16, causal, ragged N, scale 0.3
    assert all(any(c.startswith("mfma16 bfloat16 N=257") for c, _ in by) for by in caught.values())


def test_old_max_norm_bar_misses_renormalization_and_last_key():
    """the shape and inputs of test_bwd_parity.py's test_larger_sizes_vs_live_autograd_and_properties (bf16 1x8x2048x128,
    causal, spread 0.5): with the fp32 row renormalization dropped, dQ and dV stay inside |a - truth| <= 2.5e-2 max|truth|
    (only dK leaves it, narrowly); with the last key dropped all three do.  compare() fails both."""
    torch.manual_seed(11)
    Q, K, V, dO = ((torch.randn(1, 8, 2048, 128) * 0.5).to(torch.bfloat16) for _ in range(4))
    O, L = stored_forward(Q, K, V, True)
    q, k, v = (t.double().requires_grad_(True) for t in (Q, K, V))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=1.0, is_causal=True)
    truth = torch.autograd.grad(o, (q, k, v), dO.double())
    ref = A.restate(Q, K, V, O, L, dO, True, 1.0, "mfma16")
    rel = lambda g: [((a.double() - t).abs().max() / t.abs().max()).item() for a, t in zip(g, truth)]
    assert max(rel(ref[:3])) <= REL[torch.bfloat16]
    r = rel(A.restate(Q, K, V, O, L, dO, True, 1.0, "mfma16", plant="no_renorm", bars=False)[:3])
    print("no_renorm: |err| / max|truth| =", r)
    assert r[0] <= REL[torch.bfloat16] and r[2] <= REL[torch.bfloat16]
    r2 = rel(A.restate(Q, K, V, O, L, dO, True, 1.0, "mfma16", plant="drop_last_key", bars=False)[:3])
    print("drop_last_key: |err| / max|truth| =", r2)
    assert max(r2) <= REL[torch.bfloat16]
    for p in ("no_renorm", "drop_last_key"):
        bad = A.restate(Q, K, V, O, L, dO, True, 1.0, "mfma16", plant=p, bars=False)
        assert not all(ok for *_, ok in A.compare(bad[:3], ref)), p


# ----------------------------------------------------------------------------- window and varlen
def stored_forward_band(Q, K, V, keep, scale):
    """O and L of a window / rectangular (one varlen sequence) problem as the forward stores them: fp64, rounded once to the
    I/O dtype; a row without a visible key O = 0, L = +inf"""
    from oracle.fa2_mask_probe import truth
    O, L = truth(Q, K, V, keep, Q.dtype, scale)
    return O.to(Q.dtype), L.to(Q.dtype)


def rand_rect(B, H, nq, nk, d, dtype, seed, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    Q, dO = ((torch.randn(B, H, nq, d, generator=g) * spread).to(dtype) for _ in range(2))
    K, V = ((torch.randn(B, H, nk, d, generator=g) * spread).to(dtype) for _ in range(2))
    return Q, K, V, dO


# (nq, nk, window, causal): dense windows (nq = nk) and single varlen sequences, bottom-right aligned, empty rows included
BAND_PROBLEMS = [(65, 65, (16, 15), False), (130, 130, (-1, 31), False), (100, 100, (40, 0), True), (72, 72, (0, 0), False),
                 (40, 103, (31, -1), False), (103, 40, None, True), (64, 129, (1, 1), False), (129, 63, (-1, 0), False),
                 (1, 33, (15, -1), True)]


@pytest.mark.parametrize("kernel", A.KERNELS)
@pytest.mark.parametrize("problem", BAND_PROBLEMS, ids=str)
def test_band_restatement_matches_fp64_autograd(kernel, problem):
    """fp32 I/O: the restatement of a window / varlen problem against fp64 autograd through the masked softmax (rows with no
    visible key: P = 0)"""
    nq, nk, window, causal = problem
    Q, K, V, dO = rand_rect(1, 2, nq, nk, 32, torch.float32, seed=nq + nk)
    scale = 0.4
    keep = A.band(nq, nk, causal, window)
    O, L = stored_forward_band(Q, K, V, keep, scale)
    got = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, bars=False, window=window)
    q, k, v = (t.double().requires_grad_(True) for t in (Q, K, V))
    S = (q @ k.transpose(-1, -2) * scale).masked_fill(~keep, -math.inf)
    vis = keep.any(-1, keepdim=True)
    o = torch.where(vis, torch.softmax(S.masked_fill(~vis, 0.0), -1), 0.0) @ v
    truth = torch.autograd.grad(o, (q, k, v), dO.double())
    for name, a, t in zip(("dQ", "dK", "dV"), got, truth):
        assert a.dtype == torch.float32 and a.shape == t.shape
        assert (a.double() - t).abs().max() <= 1e-5 * t.abs().max() + 1e-12, name   # (+: dQ of a one-key band is 0)
    empty = ~vis[:, 0]
    assert (got[0][:, :, empty] == 0).all()            # keyless rows: dQ exactly 0, not 0 * inf
    unseen = ~keep.any(0)
    assert (got[1][:, :, unseen] == 0).all() and (got[2][:, :, unseen] == 0).all()
    same = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, bars=False, keep=keep)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], same[:3]))


# (shape (B, H, nq, nk, d), dtype, window, causal, scale, spread, kernel)
BAND_BAR_CASES = [((1, 2, 257, 257, 64), torch.bfloat16, (31, 33), False, 0.3, 0.5, "mfma16"),
                  ((1, 2, 512, 512, 128), torch.bfloat16, (128, 128), False, 1.0, 1.0, "mfma16"),
                  ((1, 2, 300, 300, 64), torch.float16, (-1, 95), False, 0.3, 0.5, "generic"),
                  ((1, 2, 129, 129, 64), torch.float16, (16, 0), True, 0.125, 0.5, "mfma16"),
                  ((1, 2, 130, 197, 64), torch.bfloat16, (63, 1), False, 0.3, 0.5, "mfma16"),      # varlen: N_k - N_q = 67
                  ((1, 2, 200, 137, 128), torch.float16, None, True, 0.3, 0.5, "mfma16"),          # 63 keyless rows
                  ((1, 2, 161, 96, 64), torch.bfloat16, (-1, 40), False, 0.3, 0.5, "generic")]


def _band_case(case):
    (B, H, nq, nk, d), dtype, window, causal, scale, spread, kernel = case
    Q, K, V, dO = rand_rect(B, H, nq, nk, d, dtype, seed=nq + 3 * nk, spread=spread)
    O, L = stored_forward_band(Q, K, V, A.band(nq, nk, causal, window), scale)
    return Q, K, V, O, L, dO


def _band_id(c):
    return f"{c[6]}-{str(c[1])[6:]}-{c[0][2]}x{c[0][3]}-w{c[2]}-causal{int(c[3])}"


@pytest.mark.parametrize("case", BAND_BAR_CASES, ids=_band_id)
def test_fp32_arithmetic_passes_the_bars_on_window_and_varlen(case):
    _, dtype, window, causal, scale, _, kernel = case
    Q, K, V, O, L, dO = _band_case(case)
    ref = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, window=window)
    assert all(torch.isfinite(t).all() for t in ref.tol)
    emu = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, bars=False, acc=torch.float32, window=window)
    A.assert_close(emu[:3], ref, case)


def test_planted_errors_fail_the_bars_on_window_and_varlen():
    """every mask plant (an edge one key out, top-left alignment) is caught on at least one window / varlen case, and
    every one of the dense plants on at least one windowed case"""
    caught = {p: [] for p in A.PLANTS + A.MASK_PLANTS}
    for case in BAND_BAR_CASES:
        _, dtype, window, causal, scale, _, kernel = case
        Q, K, V, O, L, dO = _band_case(case)
        ref = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, window=window)
        for p in caught:
            bad = A.restate(Q, K, V, O, L, dO, causal, scale, kernel, plant=p, bars=False, window=window)
            if not all(ok for *_, ok in A.compare(bad[:3], ref)):
                caught[p].append(_band_id(case))
    for p, by in caught.items():
        print(f"{p}: caught by {by}")
    assert all(caught.values()), {p: by for p, by in caught.items() if not by}
    windowed = {_band_id(c) for c in BAND_BAR_CASES if c[2] is not None and c[0][2] == c[0][3]}
    assert all(set(caught[p]) & windowed for p in A.PLANTS + ("right_plus_one", "left_minus_one")), caught
    assert not set(caught["top_left"]) & windowed            # (top-left = bottom-right when N_q = N_k)
