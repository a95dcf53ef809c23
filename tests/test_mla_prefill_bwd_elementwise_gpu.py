"""The packed backward at d 192 / d_v 128 on the GPU, element by element: forced mfma16dv, forced generic and auto on the forward's
grid with the forward's real O and L, each gradient held to oracle.fa2_bwd_arith.assert_close against the per-sequence restatement
(tests/mla_prefill_bwd_cases.py) -- its element-wise bars and its 90 % bit-identical floor for the 16-bit types."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_prefill_bwd_cases as C
from oracle import fa2_bwd_arith as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ARITH = {"mfma16dv": "mfma16", "auto": "mfma16", "generic": "generic"}   # (auto at f16 / bf16 192 / 128 is the matrix kernel)


def cu_of(lengths):
    return torch.tensor(C.starts(lengths), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def problem(dtype, dist, causal, window):
    """Q, K, V, O, L, dO on the device: the forward's own O and L, computed once per problem"""
    Q, K, V, dO = (t.to(DEV) for t in C.data(dtype, dist=dist))
    O, L = fa.flash_attention_mla_prefill_forward(Q, K, V, cu_of(C.LQ), cu_of(C.LK), max(C.LQ), max(C.LK), DEV, causal=causal,
                                                  scale=C.SCALE, window=window)
    return Q, K, V, O, L, dO


@functools.lru_cache(maxsize=None)
def reference(dtype, dist, causal, window, kernel):
    return C.reference(*problem(dtype, dist, causal, window), C.LQ, C.LK, causal, C.SCALE, window, kernel)


def check(dtype, dist, causal, window, variant):
    Q, K, V, O, L, dO = problem(dtype, dist, causal, window)
    got = fa.flash_attention_mla_prefill_backward(Q, K, V, O, dO, L, cu_of(C.LQ), cu_of(C.LK), max(C.LQ), max(C.LK), DEV, causal=causal,
                                                  scale=C.SCALE, window=window, variant=variant)
    parts, nonzero = C.split(got, C.LQ, C.LK)
    assert not nonzero, (variant, causal, window, nonzero)               # a sequence without queries or keys: zero gradients
    ref = reference(dtype, dist, causal, window, ARITH[variant])
    assert sorted(parts) == sorted(ref)
    for b in ref:
        A.assert_close(parts[b], ref[b], (variant, dist, causal, window, b))


@pytest.mark.parametrize("variant", ("mfma16dv", "generic", "auto"))
@pytest.mark.parametrize("dtype", (C.BF16, C.F16))
def test_gradients_element_wise_on_the_grid(dtype, variant):
    for causal, window in C.MASKS:
        check(dtype, "normal", causal, window, variant)


@pytest.mark.parametrize("variant", ("mfma16dv", "generic", "auto"))
@pytest.mark.parametrize("dist", ("onehot", "latemax"))
def test_gradients_element_wise_on_hard_rows(dist, variant):
    for dtype in (C.BF16, C.F16):
        for causal, window in ((True, None), (False, (100, 50))):
            check(dtype, dist, causal, window, variant)
