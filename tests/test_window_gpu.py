"""Local (sliding-window) attention on the GPU: forward O and L against the fp64 windowed truth of the rounded inputs, the
normalisation (reducing windows are bit-identical to the plain / causal calls), canary arenas, the backward against fp64 autograd
through the windowed softmax, gradcheck, determinism, head slices and one large case."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import (FlashAttention, attention_backward_recompute, convert_triton_dtype,
                                                            window_mask)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (fp64: 1e-6 -- the windowed VALU kernel was measured at up to 5e-8 against torch's fp64 softmax at N = 2065, 1e-16 at N <= 1000; a
# masking error moves O by O(0.1))
O_TOL = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 5e-2, torch.float64: 1e-6}
FP8_STEP = {torch.float8_e5m2: 0.25, torch.float8_e4m3fn: 0.125}
BWD_REL = {torch.float16: 4e-3, torch.bfloat16: 2.5e-2, torch.float32: 2e-4, torch.float64: 1e-6}
NS = (1, 31, 64, 200, 256, 1000, 2065)
WINDOWS = ((0, 0), (1, 0), (0, 1), (31, 0), (32, 0), (63, 64), (127, 0), (128, 128), (300, -1), (-1, 300))


def f32(x):  # the ABI takes the softmax scale as a float
    return float(torch.tensor(x, dtype=torch.float32))


def truth(Q, K, V, causal, scale, window):
    scale = f32(scale)
    q, k, v = (t.to(DEV).double() for t in (Q, K, V))
    S = torch.matmul(q, k.transpose(-1, -2)) * scale
    mask = window_mask(Q.shape[2], causal, window, DEV)
    if mask is not None:
        S = S.masked_fill(~mask, float("-inf"))
    return torch.matmul(torch.softmax(S, -1), v), torch.logsumexp(S, -1, keepdim=True) * math.log2(math.e)


def ulp(dtype, x):
    mant = {torch.float16: 10, torch.bfloat16: 7}[dtype]
    return 2.0 ** (math.floor(math.log2(max(abs(x), 1e-30))) - mant)


def check(O, L, O_ref, L_ref, dtype, what):
    O, L = O.double(), L.double()
    assert torch.isfinite(O).all() and torch.isfinite(L).all(), what
    if dtype in FP8_STEP:
        step = FP8_STEP[dtype]
        assert (O - O_ref).abs().max() <= 2 * step * max(1.0, O_ref.abs().max().item()), what
        assert (L - L_ref).abs().max() <= step * max(1.0, L_ref.abs().max().item()), what
        return
    assert (O - O_ref).abs().max() <= O_TOL[dtype], what
    if dtype in (torch.float32, torch.float64):
        assert ((L - L_ref).abs() <= 5e-5 * L_ref.abs().clamp(min=1)).all(), what
    else:
        assert (L - L_ref).abs().max() <= 1.01 * ulp(dtype, L_ref.abs().max().item()), what


def inputs(shape, dtype, seed, amp=0.5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(*shape, generator=g) * amp).to(dtype).to(DEV) for _ in range(3)]


CASES = [(dt, "generic", d) for dt in (torch.float64, torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn,
                                       torch.float8_e5m2) for d in (64, 128)]
CASES += [(dt, v, d) for dt in (torch.float16, torch.bfloat16) for v in ("auto", "mfma16d", "mfma16d_w4") for d in (64, 128)]
CASES += [(torch.float32, "auto", 64), (torch.float8_e4m3fn, "auto", 128)]


@pytest.mark.parametrize("dtype,variant,d", CASES)
def test_forward_window_against_fp64_truth(dtype, variant, d):
    scale = 1.0 / math.sqrt(d) if d == 128 else 0.7
    for N in NS:
        if dtype in (torch.float64, torch.float32, torch.float8_e4m3fn, torch.float8_e5m2) and N > 1000 and d == 128:
            continue  # (the VALU kernel at the long shape: covered at d = 64)
        Q, K, V = inputs((1, 2, N, d), dtype, N + d)
        for window in WINDOWS:
            for causal in (False, True):
                O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale, variant=variant, window=window)
                O_ref, L_ref = truth(Q, K, V, causal, scale, window)
                check(O, L, O_ref, L_ref, dtype, (variant, N, window, causal))


@pytest.mark.parametrize("d", [40, 96])
def test_forward_window_padded_head_sizes_and_strided_layout(d):
    B, N, H = 2, 300, 3
    for dtype in (torch.bfloat16, torch.float16):
        Qb, Kb, Vb = inputs((B, N, H, d), dtype, d)  # (B, N, H, d) storage, (B, H, N, d) views
        Q, K, V = (t.transpose(1, 2) for t in (Qb, Kb, Vb))
        for window, causal in (((17, 0), True), ((40, 9), False)):
            O = FlashAttention.apply(Q, K, V, causal, 0.4, window)
            O_ref, _ = truth(Q, K, V, causal, 0.4, window)
            assert O.shape == Q.shape
            assert (O.double() - O_ref).abs().max() <= O_TOL[dtype], (d, dtype, window)
            O2, L2 = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=0.4, window=window)
            assert O2.is_contiguous() and torch.equal(O2, O.contiguous())


def test_reducing_windows_are_bit_identical_to_plain_and_causal():
    for dtype, d, N in ((torch.bfloat16, 128, 512), (torch.float16, 64, 300), (torch.float32, 64, 200)):
        Q, K, V = inputs((2, 2, N, d), dtype, 7)
        plain = fa.flash_attention_forward(Q, K, V, DEV)
        causal = fa.flash_attention_forward(Q, K, V, DEV, causal=True)
        for window, c, ref in (((-1, -1), False, plain), ((N - 1, N - 1), False, plain), ((-1, 0), False, causal),
                               ((-1, 5), True, causal), ((N + 4, -1), True, causal)):
            O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=c, window=window)
            assert torch.equal(O, ref[0]) and torch.equal(L, ref[1]), (dtype, window, c)
            # the C layer normalises too: fa2_fwd_window straight from the ABI
            O2, L2 = torch.empty_like(ref[0]), torch.empty_like(ref[1])
            _lib.fa2_fwd(Q, K, V, O2, L2, convert_triton_dtype(dtype), causal=c, window=window)
            assert torch.equal(O2, ref[0]) and torch.equal(L2, ref[1]), (dtype, window, c)
        dO = inputs((2, 2, N, d), dtype, 8)[0]
        O, L = causal
        g_ref = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=True)
        g = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, window=(-1, 0))
        assert all(torch.equal(a, b) for a, b in zip(g, g_ref))


SENT = {torch.bfloat16: -12345.0, torch.float32: -12345.0, torch.float16: -1234.0}


@pytest.mark.parametrize("dtype,fvar,bvar", [(torch.bfloat16, "mfma16d", "mfma16"), (torch.float16, "mfma16d_w4", "mfma16"),
                                             (torch.float32, "generic", "generic"), (torch.bfloat16, "generic", "generic")])
def test_canary_arenas(dtype, fvar, bvar):
    B, H, N, d = 1, 2, 333, 64
    Q, K, V = inputs((B, H, N, d), dtype, 3)
    window = (70, 5)

    def arena(rows, cols):  # logical (B, H, N, cols) inside a larger buffer: pad rows before/after, extra columns
        buf = torch.full((B, H, rows + 8, cols + 16), SENT[dtype], dtype=dtype, device=DEV)
        return buf, buf[:, :, 4:4 + rows, 8:8 + cols]

    Ob, O = arena(N, d)
    Lb = torch.full((B, H, N + 8), SENT[dtype], dtype=dtype, device=DEV)  # L: unit stride over N
    L = Lb[:, :, 4:4 + N].unsqueeze(-1)
    _lib.fa2_fwd(Q, K, V, O, L, convert_triton_dtype(dtype), variant=_lib.VARIANTS[fvar], window=window)
    outside = Ob.clone()
    outside[:, :, 4:4 + N, 8:8 + d] = SENT[dtype]
    assert (outside == SENT[dtype]).all()
    outside = Lb.clone()
    outside[:, :, 4:4 + N] = SENT[dtype]
    assert (outside == SENT[dtype]).all()
    O_ref, L_ref = truth(Q, K, V, False, 1.0, window)
    check(O, L, O_ref, L_ref, dtype, "canary")
    dO = inputs((B, H, N, d), dtype, 4)[0]
    grads = [arena(N, d) for _ in range(3)]
    D = torch.empty(2, B, H, N, 1, dtype=torch.float32, device=DEV)
    _lib.fa2_bwd(Q, K, V, O, dO, L, grads[0][1], grads[1][1], grads[2][1], D, convert_triton_dtype(dtype),
                 variant=_lib.BWD_VARIANTS[bvar], window=window)
    for buf, view in grads:
        outside = buf.clone()
        outside[:, :, 4:4 + N, 8:8 + d] = SENT[dtype]
        assert (outside == SENT[dtype]).all()
        assert torch.isfinite(view).all()


def grads_truth(Q, K, V, dO, causal, scale, window):
    scale = f32(scale)
    q, k, v = (t.detach().double().requires_grad_() for t in (Q, K, V))
    S = torch.matmul(q, k.transpose(-1, -2)) * scale
    mask = window_mask(Q.shape[2], causal, window, DEV)
    if mask is not None:
        S = S.masked_fill(~mask, float("-inf"))
    O = torch.matmul(torch.softmax(S, -1), v)
    O.backward(dO.double())
    return q.grad, k.grad, v.grad


@pytest.mark.parametrize("dtype,variant,d", [(torch.bfloat16, "mfma16", 128), (torch.float16, "mfma16", 64),
                                             (torch.bfloat16, "generic", 64), (torch.float32, "generic", 64),
                                             (torch.float64, "generic", 32), (torch.float16, "auto", 128)])
def test_backward_window_against_fp64_autograd(dtype, variant, d):
    scale = 1.0 / math.sqrt(d)
    for N in (31, 200, 1000):
        Q, K, V = inputs((1, 2, N, d), dtype, N, amp=0.8)
        dO = inputs((1, 2, N, d), dtype, N + 1)[0]
        for window in ((0, 0), (31, 0), (63, 64), (128, 128), (300, -1), (-1, 300)):
            for causal in (False, True):
                O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale, window=window)
                g = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=scale, variant=variant,
                                                window=window)
                t = grads_truth(Q, K, V, dO, causal, scale, window)
                for name, a, b in zip("QKV", g, t):
                    assert torch.isfinite(a).all()
                    err = (a.double() - b).abs().max().item()
                    assert err <= BWD_REL[dtype] * max(1.0, b.abs().max().item()), (variant, N, window, causal, name, err)
                if dtype in (torch.float32, torch.float64):  # the torch recompute path agrees with the kernels
                    r = attention_backward_recompute(Q, K, V, O, dO, L, causal, scale, window=window)
                    for a, b in zip(g, r):
                        assert (a.double() - b.double()).abs().max() <= 1e-3 * max(1.0, b.abs().max().item())


def test_gradcheck_f64():
    for window, causal in (((2, 1), False), ((3, 0), True), ((0, 0), False)):
        Q, K, V = (torch.randn(1, 1, 9, 16, dtype=torch.float64, device=DEV, requires_grad=True) for _ in range(3))
        f = lambda q, k, v: FlashAttention.apply(q, k, v, causal, 0.5, window)  # noqa: E731
        assert torch.autograd.gradcheck(f, (Q, K, V), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_apply_arities():
    Q, K, V = inputs((1, 2, 64, 64), torch.float32, 2)
    for args in ((), (True, 0.5), (True, 0.5, (8, 0)), (False, 1.0, None)):
        qs = [t.clone().requires_grad_() for t in (Q, K, V)]
        O = fa.FlashAttentionDeterministic.apply(*qs, *args)
        O.sum().backward()
        assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in qs)


def test_determinism_and_head_slices():
    B, H, N, d = 2, 4, 777, 128
    Q, K, V = inputs((B, H, N, d), torch.bfloat16, 11)
    dO = inputs((B, H, N, d), torch.bfloat16, 12)[0]
    window = (100, 0)
    O, L = fa.flash_attention_forward(Q, K, V, DEV, window=window)
    g = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, window=window)
    O2, L2 = fa.flash_attention_forward(Q, K, V, DEV, window=window)
    g2 = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, window=window)
    assert torch.equal(O, O2) and torch.equal(L, L2) and all(torch.equal(a, b) for a, b in zip(g, g2))
    sl = slice(1, 3)
    Os, Ls = fa.flash_attention_forward(Q[:, sl], K[:, sl], V[:, sl], DEV, window=window)
    gs = fa.flash_attention_backward(Q[:, sl], K[:, sl], V[:, sl], O[:, sl], dO[:, sl], L[:, sl], DEV, window=window)
    assert torch.equal(Os, O[:, sl]) and torch.equal(Ls, L[:, sl])
    assert all(torch.equal(a, b[:, sl]) for a, b in zip(gs, g))


def test_large_benchmarked_case():
    """bf16 B4 H32 N16384 d128, window (1024, 0) causal: sampled heads against an fp32 blockwise reference on the GPU"""
    B, H, N, d = 4, 32, 16384, 128
    window, scale = (1024, 0), 1.0 / math.sqrt(d)
    Q, K, V, dO = ((torch.randn(B, H, N, d, device=DEV) * 0.8).to(torch.bfloat16) for _ in range(4))
    O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=True, scale=scale, window=window)
    g = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=True, scale=scale, window=window)
    for t in (O, L, *g):
        assert torch.isfinite(t).all()
    for b, h in ((0, 0), (3, 31), (2, 17)):
        q, k, v = (t[b, h].float() for t in (Q, K, V))
        for r0 in (0, 5000, N - 2048):  # blockwise: 2048 query rows against their band of keys
            rows = torch.arange(r0, r0 + 2048, device=DEV)
            k0 = max(0, r0 - window[0])
            S = (q[r0:r0 + 2048] @ k[k0:r0 + 2048].T) * scale
            j = torch.arange(k0, r0 + 2048, device=DEV)
            vis = (j[None, :] >= rows[:, None] - window[0]) & (j[None, :] <= rows[:, None])
            S = S.masked_fill(~vis, float("-inf"))
            O_ref = torch.softmax(S, -1) @ v[k0:r0 + 2048]
            L_ref = torch.logsumexp(S, -1) * math.log2(math.e)
            assert (O[b, h, r0:r0 + 2048].float() - O_ref).abs().max() <= O_TOL[torch.bfloat16]
            assert (L[b, h, r0:r0 + 2048, 0].float() - L_ref).abs().max() <= 1.01 * ulp(torch.bfloat16, L_ref.abs().max().item())
