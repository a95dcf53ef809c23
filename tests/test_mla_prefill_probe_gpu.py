"""The exact-arithmetic probe of tests/mla_prefill_probe.py through the Python surface of the packed forward at d = 192 / d_v = 128
(flash_attention_mla_prefill_forward): f16 / bf16 under auto, the matrix kernel and the VALU kernel, f32 under the VALU kernel; H 4
with H_kv 4, 2 and 1, causal on and off, four windows, sequence lengths on every edge of the 128-row query tile and the 64-key unit.
The bars are the probe's (one output ulp on O and L, exact zeros, exact empty rows; float32 4 ulps), proven on the CPU by
tests/test_mla_prefill_probe.py."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_prefill_probe as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@functools.lru_cache(maxsize=None)
def probe(h_kv, uniform):
    return M.inputs(h_kv, uniform, DEV)


@functools.lru_cache(maxsize=None)
def truth(h_kv, uniform, causal, window):
    """the fp64 truth at c = 1 (the same for every dtype of this grid), computed once and shared"""
    return M.reference(*probe(h_kv, uniform), h_kv, M.keep_of(causal, window, device=DEV), F32)


def cu_of(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


FWD = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mfma16dv", "generic")] + [(F32, "generic")]


@pytest.mark.parametrize("h_kv", M.H_KVS)
@pytest.mark.parametrize("dtype,variant", FWD)
def test_mla_prefill_probe(dtype, variant, h_kv):
    cu_q, cu_k = cu_of(M.LQ), cu_of(M.LK)
    for uniform in (False, True):
        Q, K, V = (t.to(dtype) for t in probe(h_kv, uniform))
        for _, causal, window in (c for c in M.cases() if c[0] == h_kv):
            O, L = fa.flash_attention_mla_prefill_forward(Q, K, V, cu_q, cu_k, max(M.LQ), max(M.LK), DEV, causal=causal,
                                                          scale=M.SCALE, window=window, variant=variant)
            assert O.shape == (sum(M.LQ), M.H, M.D_V) and O.is_contiguous() and L.shape == (M.H, sum(M.LQ))
            v = M.violations_of(O, L, *truth(h_kv, uniform, causal, window), dtype)
            assert not v, (uniform, causal, window, v)
