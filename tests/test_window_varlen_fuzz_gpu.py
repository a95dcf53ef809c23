"""Seeded random sweep of windowed and varlen attention on the GPU, in the style of tests/test_fuzz_gpu.py: each case draws
B, H, N or a length mix, d, dtype, window sides and causal, and runs three checks -- the forward through the exact mask
probe (oracle/fa2_mask_probe.py), the forward on random inputs against fp64 truth at the bars of tests/test_window_gpu.py,
and the backward element-wise against oracle/fa2_bwd_arith.restate.  Seeded: the same cases every run
(oracle/fa2_mask_probe.fuzz_window_cases / fuzz_varlen_cases, whose probe cases tests/test_mask_probe.py proves)."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from oracle import fa2_bwd_arith as A
from flash_attention_dlrs_amd.flash_attention_torch import normalize_window
from oracle import fa2_mask_probe as P
from test_bwd_elementwise import auto_kernel
from test_window_varlen_bwd_gpu import check_varlen

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
O_TOL = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 5e-2}     # tests/test_window_gpu.py
def _kernel(dtype, d):
    """the windowed / varlen backward's auto choice (fa2_bwd_api.hip run_window, the varlen run)"""
    return "mfma16" if dtype in (torch.float16, torch.bfloat16) and d in (64, 128) else "generic"


def _window_kernel(N, causal, window, dtype, d, scale):
    """a window that normalises to plain or causal attention takes the dense backward, whose auto choice differs (mfma32
    for fp32 at d 64 / 128)"""
    return _kernel(dtype, d) if normalize_window(N, causal, window)[1] is not None else auto_kernel(dtype, d, scale)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


@pytest.mark.parametrize("B,H,N,d,dtype,window,causal,scale", P.fuzz_window_cases(), ids=lambda v: str(v).replace("torch.", ""))
def test_random_window(B, H, N, d, dtype, window, causal, scale):
    keep = P.dense_keep(N, causal, window, device=DEV)
    for uniform in (False, True):
        Q, K, V = P.dense_inputs(B, H, N, d, dtype, uniform, DEV)
        O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=P.SCALE, window=window)
        O_ref, L_ref = P.truth(Q, K, V, keep, dtype)
        viol = P.violations(O, L, O_ref, L_ref, dtype)
        assert not viol, ("probe", uniform, viol)

    g = torch.Generator(device=DEV).manual_seed(B * 1000003 + H * 10007 + N * 101 + d)
    Q, K, V, dO = ((torch.randn(B, H, N, d, generator=g, device=DEV) * 0.6).to(dtype) for _ in range(4))
    O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale, window=window)
    S = (Q.double() @ K.double().transpose(-1, -2) * _f32(scale)).masked_fill(~keep, -math.inf)
    assert (O.double() - torch.softmax(S, -1) @ V.double()).abs().max() <= O_TOL[dtype]

    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=scale, window=window)
    kernel = _window_kernel(N, causal, window, dtype, d, scale)
    A.assert_close(got, A.restate(Q, K, V, O, L, dO, causal, scale, kernel, window=window), ("bwd", kernel))


@pytest.mark.parametrize("lq,lk,H,d,dtype,window,causal,scale", P.fuzz_varlen_cases(), ids=lambda v: str(v).replace("torch.", ""))
def test_random_varlen(lq, lk, H, d, dtype, window, causal, scale):
    cu_q = torch.tensor(P._cu(lq), dtype=torch.int32, device=DEV)
    cu_k = torch.tensor(P._cu(lk), dtype=torch.int32, device=DEV)
    mq, mk = max(lq), max(lk)
    keep = P.varlen_keep(lq, lk, causal, window, device=DEV)
    for uniform in (False, True):
        Q, K, V = P.varlen_inputs(lq, lk, H, d, dtype, uniform, DEV)
        O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, mq, mk, DEV, causal=causal, scale=P.SCALE,
                                                 window=window)
        O_ref, L_ref = P.truth(*P.heads_first(Q, K, V), keep, dtype)
        viol = P.violations(O.transpose(0, 1), L, O_ref, L_ref, dtype)
        assert not viol, ("probe", uniform, viol)

    g = torch.Generator(device=DEV).manual_seed(sum(lq) * 1009 + sum(lk) * 31 + d)
    tq, tk = sum(lq), sum(lk)
    Q, dO = ((torch.randn(tq, H, d, generator=g, device=DEV) * 0.6).to(dtype) for _ in range(2))
    K, V = ((torch.randn(tk, H, d, generator=g, device=DEV) * 0.6).to(dtype) for _ in range(2))
    O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, mq, mk, DEV, causal=causal, scale=scale, window=window)
    S = (torch.einsum("qhd,khd->hqk", Q.double(), K.double()) * _f32(scale)).masked_fill(~keep, -math.inf)
    vis = keep.any(-1, keepdim=True)
    Pm = torch.where(vis, torch.softmax(S.masked_fill(~vis, 0.0), -1), 0.0)
    O_t = torch.einsum("hqk,khd->qhd", Pm, V.double())
    assert (O.double() - O_t).abs().max() <= O_TOL[dtype]

    got = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, mq, mk, DEV, causal=causal, scale=scale,
                                             window=window)
    check_varlen(Q, K, V, O, L, dO, got, lq, lk, causal, scale, window, _kernel(dtype, d), "fuzz")
