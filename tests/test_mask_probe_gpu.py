"""Every windowed and varlen forward form through the exact-arithmetic mask probe (oracle/fa2_mask_probe.py): O within one
output ulp of the fp64 truth, exact zeros where no visible key writes, L within one ulp, empty varlen rows O = 0 and L = +inf.
tests/test_mask_probe.py shows on the CPU that a band one key off fails these bars on every case run here."""
import pytest
import torch

import flash_attention_dlrs_amd as fa
from oracle import fa2_mask_probe as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F8 = (torch.float8_e4m3fn, torch.float8_e5m2)

FWD = [(dt, v, d) for dt in (torch.float16, torch.bfloat16) for v in ("auto", "generic", "mfma16d", "mfma16d_w4")
       for d in (64, 128)]
FWD_VALU = [(dt, "generic", d) for dt in (torch.float32, torch.float64) for d in (64, 128)]


def _dense(dtype, variant, d, cases, B=1, H=2):
    bad = []
    for N, window, causal in cases:
        keep = P.dense_keep(N, causal, window, device=DEV)
        for uniform in (False, True):
            Q, K, V = P.dense_inputs(B, H, N, d, dtype, uniform, DEV)
            O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=P.SCALE, variant=variant, window=window)
            O_ref, L_ref = P.truth(Q, K, V, keep, dtype)
            v = P.violations(O, L, O_ref, L_ref, dtype)
            if v:
                bad.append((N, window, causal, uniform, v))
    return bad


@pytest.mark.parametrize("dtype,variant,d", FWD + FWD_VALU, ids=lambda x: str(x).replace("torch.", ""))
def test_window_probe(dtype, variant, d):
    bad = _dense(dtype, variant, d, P.window_cases())
    assert not bad, bad[:10]


@pytest.mark.parametrize("dtype", F8)
@pytest.mark.parametrize("d", [64, 128])
def test_window_probe_fp8(dtype, d):
    cases = [c for c in P.window_cases() if P.fp8_applies(c[1], c[2], d)]
    assert len(cases) >= 5
    bad = _dense(dtype, "generic", d, cases)
    assert not bad, bad[:10]


def _varlen(dtype, variant, d, cases, H=2):
    bad = []
    for lq, lk, window, causal in cases:
        keep = P.varlen_keep(lq, lk, causal, window, device=DEV)
        cu_q = torch.tensor(P._cu(lq), dtype=torch.int32, device=DEV)
        cu_k = torch.tensor(P._cu(lk), dtype=torch.int32, device=DEV)
        for uniform in (False, True):
            Q, K, V = P.varlen_inputs(lq, lk, H, d, dtype, uniform, DEV)
            O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, max(lq), max(lk), DEV, causal=causal,
                                                     scale=P.SCALE, window=window, variant=variant)
            O_ref, L_ref = P.truth(*P.heads_first(Q, K, V), keep, dtype)
            v = P.violations(O.transpose(0, 1), L, O_ref, L_ref, dtype)
            if v:
                bad.append((lq, lk, window, causal, uniform, v))
    return bad


VARLEN = FWD + [(dt, v, 64) for dt in (torch.float32, torch.float64) for v in ("auto", "generic")]


@pytest.mark.parametrize("dtype,variant,d", VARLEN, ids=lambda x: str(x).replace("torch.", ""))
def test_varlen_probe(dtype, variant, d):
    bad = _varlen(dtype, variant, d, P.varlen_cases())
    assert not bad, bad[:10]


@pytest.mark.parametrize("d", [40, 64, 96, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_probe_strided_views_and_padded_head_sizes(dtype, d):
    """B 2 H 3: (B, N, H, d) storage viewed as (B, H, N, d) through the Python surface (d 40 / 96 are padded by it), and
    a packed batch at H 3 read from a strided (total, 3, H, d) buffer"""
    bad = []
    for N, window, causal in P.LAYOUT_CASES:
        keep = P.dense_keep(N, causal, window, device=DEV)
        for uniform in (False, True):
            Qc, Kc, Vc = P.dense_inputs(2, 3, N, d, dtype, uniform, DEV)
            Q, K, V = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (Qc, Kc, Vc))
            assert Q.stride(1) == d and not Q.is_contiguous()
            O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=P.SCALE, window=window)
            O_ref, L_ref = P.truth(Qc, Kc, Vc, keep, dtype)
            v = P.violations(O, L, O_ref, L_ref, dtype)
            O2 = fa.FlashAttention.apply(Q, K, V, causal, P.SCALE, window)
            if v or not torch.equal(O2.contiguous(), O.contiguous()):
                bad.append((N, window, causal, uniform, v))
    lq, lk, windows = P.LAYOUT_VARLEN
    for window, causal in windows:
        keep = P.varlen_keep(lq, lk, causal, window, device=DEV)
        q, k, v = P.varlen_inputs(lq, lk, 3, d, dtype, False, DEV)
        tq, tk = sum(lq), sum(lk)
        buf = torch.zeros(max(tq, tk), 3, 3, d, dtype=dtype, device=DEV)
        buf[:tq, 0], buf[:tk, 1], buf[:tk, 2] = q, k, v
        Q, K, V = buf[:tq, 0], buf[:tk, 1], buf[:tk, 2]
        cu_q = torch.tensor(P._cu(lq), dtype=torch.int32, device=DEV)
        cu_k = torch.tensor(P._cu(lk), dtype=torch.int32, device=DEV)
        O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, max(lq), max(lk), DEV, causal=causal, scale=P.SCALE,
                                                 window=window)
        O_ref, L_ref = P.truth(*P.heads_first(q, k, v), keep, dtype)
        viol = P.violations(O.transpose(0, 1), L, O_ref, L_ref, dtype)
        if viol:
            bad.append(("varlen", window, causal, viol))
    assert not bad, bad
