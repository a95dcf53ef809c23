"""The windowed and varlen backward kernels (mfma16, generic and the auto choice) element by element against
oracle/fa2_bwd_arith.restate, fed with the forward's real O and L: the bars and the bit-identical fraction of
tests/test_bwd_elementwise.py, on the band the problem defines (per sequence for varlen).  Keys no query sees get exactly
zero dK and dV; rows with no visible key exactly zero dQ."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd.flash_attention_torch import normalize_window
from oracle import fa2_bwd_arith as A
from oracle import fa2_mask_probe as P
from test_bwd_elementwise import DISTS, auto_kernel, draw

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (window, N): boundary windows, and the wide windows of the issue's table -- (128, 128), (-1, 300) -- at N = 1000, where a
# one-key error used to pass the autograd bars.  Every case is a real window at its N (not reduced to plain or causal
# attention by normalize_window, which would run the dense kernels of tests/test_bwd_elementwise.py instead); causal runs
# only where the left side is bounded (causal with an unbounded left side is causal attention)
WINDOWS = [((0, 0), 65), ((1, 0), 33), ((16, 15), 129), ((31, 33), 65), ((32, 32), 257), ((63, 64), 129), ((65, -1), 257),
           ((-1, 95), 300), ((127, 129), 1000), ((128, 128), 1000), ((-1, 300), 1000), ((300, -1), 1000), ((256, 1), 513),
           ((17, 255), 257)]
COMBOS = [(dt, d, v) for dt in (torch.float16, torch.bfloat16) for d in (64, 128) for v in ("mfma16", "generic", "auto")]


def _scale(k, d):
    return (1.0, 1 / math.sqrt(d), 0.3)[k % 3]


def _kernel(variant, dtype, d, scale):
    return auto_kernel(dtype, d, scale) if variant == "auto" else variant


@pytest.mark.parametrize("dtype,d,variant", COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_window_backward_elementwise(dtype, d, variant):
    for k, (window, N) in enumerate(WINDOWS):
        for causal in (False, True) if window[0] >= 0 else (False,):
            assert normalize_window(N, causal, window)[1] is not None, (window, N, causal)
            dist, scale = DISTS[(k + 2 * causal) % 4], _scale(k, d)
            Q, K, V, dO = draw(1, 2, N, d, dtype, dist, seed=100 * k + causal)
            O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale, window=window)
            got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=scale, variant=variant,
                                              window=window)
            ref = A.restate(Q, K, V, O, L, dO, causal, scale, _kernel(variant, dtype, d, scale), window=window)
            A.assert_close(got, ref, (variant, N, window, causal, dist, scale))


def cu_of(lengths):
    return torch.tensor(P._cu(lengths), dtype=torch.int32, device=DEV)


def check_varlen(Q, K, V, O, L, dO, got, lq, lk, causal, scale, window, kernel, what):
    """per sequence against restate; unseen keys and keyless rows exactly zero"""
    dQ, dK, dV = got
    cq, ck = P._cu(lq), P._cu(lk)
    seq = lambda t, a, n: t[a:a + n].transpose(0, 1).unsqueeze(0)         # (1, H, n, d)
    for b, (nq, nk) in enumerate(zip(lq, lk)):
        qs, ks = slice(cq[b], cq[b] + nq), slice(ck[b], ck[b] + nk)
        if nq == 0 or nk == 0:
            assert (dQ[qs] == 0).all() and (dK[ks] == 0).all() and (dV[ks] == 0).all(), (what, b)
            continue
        keep = A.band(nq, nk, causal, window, DEV)
        ref = A.restate(seq(Q, cq[b], nq), seq(K, ck[b], nk), seq(V, ck[b], nk), seq(O, cq[b], nq),
                        L[:, cq[b]:cq[b] + nq].unsqueeze(0), seq(dO, cq[b], nq), causal, scale, kernel, window=window)
        A.assert_close(tuple(seq(g, a, n) for g, a, n in ((dQ, cq[b], nq), (dK, ck[b], nk), (dV, ck[b], nk))), ref,
                       (what, b, nq, nk))
        unseen = ~keep.any(0)
        assert (dK[ks][unseen] == 0).all() and (dV[ks][unseen] == 0).all(), (what, b)
        assert (dQ[qs][~keep.any(1)] == 0).all(), (what, b)


VARLEN_WINDOWS = [(None, False), (None, True), ((0, 0), False), ((15, 17), False), ((63, -1), False), ((-1, 64), False),
                  ((127, 129), False), ((31, 33), True), ((128, 128), False), ((-1, 1), False)]


def run_varlen(dtype, d, variant, lq, lk, window, causal, dist, scale, seed, H=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    sp = 1.0 if dist == "normal" else 0.5
    tq, tk = sum(lq), sum(lk)
    Q, dO = (torch.randn(tq, H, d, generator=g, device=DEV) * sp for _ in range(2))
    K, V = (torch.randn(tk, H, d, generator=g, device=DEV) * sp for _ in range(2))
    if dist == "onehot" and tq == tk:
        K = K * 0.25 + Q * 3.0
    Q, K, V, dO = (t.to(dtype) for t in (Q, K, V, dO))
    cu_q, cu_k = cu_of(lq), cu_of(lk)
    O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, max(lq), max(lk), DEV, causal=causal, scale=scale,
                                             window=window)
    got = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, max(lq), max(lk), DEV, causal=causal,
                                             scale=scale, window=window, variant=variant)
    check_varlen(Q, K, V, O, L, dO, got, lq, lk, causal, scale, window, _kernel(variant, dtype, d, scale),
                 (variant, str(dtype), d, window, causal, dist, scale))


@pytest.mark.parametrize("dtype,d,variant", COMBOS, ids=lambda x: str(x).replace("torch.", ""))
def test_varlen_backward_elementwise(dtype, d, variant):
    for m, (lq, lk) in enumerate(P.VARLEN_MIXES):
        for w in range(len(VARLEN_WINDOWS)):
            if (w + m) % 2:
                continue
            window, causal = VARLEN_WINDOWS[w]
            k = m + w
            run_varlen(dtype, d, variant, lq, lk, window, causal, DISTS[k % 3 + 1], _scale(k, d), seed=10 * m + w)
