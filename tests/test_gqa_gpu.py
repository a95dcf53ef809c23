"""Grouped-query and multi-query attention on the GPU: forward O and L and the gradients against the fp64 truth of the expanded
problem, bit identity with the MHA call on K.repeat_interleave(g, 1) under the same forced variant, H_kv == H through the new
entry points equal to the old ones, deterministic dK / dV of K's shape, canary arenas, autograd and gradcheck, and varlen GQA
(N_q != N_k, empty rows, equal-length packing equal to the dense call)."""
import ctypes
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import (FlashAttention, FlashAttentionDeterministic, FlashAttentionVarlen,
                                                            backward_native, convert_triton_dtype, expand_kv, group_sum,
                                                            varlen_backward, varlen_forward, varlen_mask, window_mask)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the bars of tests/test_window_gpu.py
O_TOL = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 5e-2, torch.float64: 1e-6}
FP8_STEP = {torch.float8_e5m2: 0.25, torch.float8_e4m3fn: 0.125}
BWD_REL = {torch.float16: 4e-3, torch.bfloat16: 2.5e-2, torch.float32: 2e-4, torch.float64: 1e-6}


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


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


def make(B, H, H_kv, N, d, dtype, layout, seed, amp=0.5):
    """Q (B, H, N, d) and K, V (B, H_kv, N, d) in `layout`, plus the MHA K, V expanded to H heads in the same layout."""
    g = torch.Generator().manual_seed(seed)
    bnhd = layout in ("b1view", "bnhd")
    def mk(h):
        shape = (B, N, h, d) if bnhd else (B, h, N, d)
        return (torch.randn(*shape, generator=g) * amp).to(dtype).to(DEV)
    Qs, Ks, Vs = mk(H), mk(H_kv), mk(H_kv)
    hdim = 2 if bnhd else 1
    Kx, Vx = (t.repeat_interleave(H // H_kv, dim=hdim) for t in (Ks, Vs))
    if bnhd:
        Qs, Ks, Vs, Kx, Vx = (t.transpose(1, 2) for t in (Qs, Ks, Vs, Kx, Vx))
    return Qs, Ks, Vs, Kx, Vx


def truth(Q, K, V, causal, scale, window):
    q, k, v = (t.double() for t in (Q, expand_kv(K, Q.shape[1]), expand_kv(V, Q.shape[1])))
    S = torch.matmul(q, k.transpose(-1, -2)) * f32(scale)
    mask = window_mask(Q.shape[2], causal, window, DEV)
    if mask is not None:
        S = S.masked_fill(~mask, float("-inf"))
    return torch.matmul(torch.softmax(S, -1), v), torch.logsumexp(S, -1, keepdim=True) * math.log2(math.e)


def grads_truth(Q, K, V, dO, causal, scale, window):
    q, k, v = (t.detach().double().requires_grad_() for t in (Q, K, V))
    S = torch.matmul(q, expand_kv(k, Q.shape[1]).transpose(-1, -2)) * f32(scale)
    mask = window_mask(Q.shape[2], causal, window, DEV)
    if mask is not None:
        S = S.masked_fill(~mask, float("-inf"))
    torch.matmul(torch.softmax(S, -1), expand_kv(v, Q.shape[1])).backward(dO.double())
    return q.grad, k.grad, v.grad


B16, F16, F32, F64, E4 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.float8_e4m3fn
# (dtype, d, variants): every variant that runs the problem
FWD = [(B16, 128, ("auto", "a64", "a16", "mfma16", "mfma16d", "mfma16d_w4", "generic")),
       (F16, 64, ("auto", "a64d", "mfma16d", "mfma16k", "generic")),
       (F32, 64, ("auto", "mfma32", "generic")),
       (E4, 128, ("auto", "a8", "mfma8x", "generic")),
       (B16, 40, ("auto", "generic"))]
WINDOWED = ("auto", "mfma16d", "mfma16d_w4", "generic")  # variants that take a window / a non-mergeable layout
LAYOUTS = (("contig", 2), ("b1view", 1), ("bnhd", 2))


def _runs(variant, dtype, d, N, layout, window):
    if window is not None or layout == "bnhd":
        if variant not in WINDOWED:
            return False
        return variant in ("auto", "generic") or (dtype in (B16, F16) and d in (64, 128))
    if variant in ("a64", "a16", "a64d", "a8"):
        return N >= 256
    return True


@pytest.mark.parametrize("dtype,d,variants", FWD)
@pytest.mark.parametrize("layout,B", LAYOUTS)
def test_forward_against_truth_and_bit_identical_to_expanded_mha(dtype, d, variants, layout, B):
    H = 8
    scale = 1.0 / math.sqrt(d)
    for N in (200, 1000):
        for H_kv in (8, 4, 2, 1):  # g = 1, 2, 4, 8 = H (MQA)
            Q, K, V, Kx, Vx = make(B, H, H_kv, N, d, dtype, layout, N + H_kv + d)
            for causal, window in ((False, None), (True, None), (False, (63, 64)), (True, (128, 0))):
                if dtype in (F32, E4) and window is not None and N > 200:
                    continue
                O_ref, L_ref = truth(Q, K, V, causal, scale, window)
                for variant in variants:
                    if not _runs(variant, dtype, d, N, layout, window):
                        continue
                    what = (layout, N, H_kv, causal, window, variant)
                    O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale, variant=variant, window=window)
                    check(O, L, O_ref, L_ref, dtype, what)
                    Om, Lm = fa.flash_attention_forward(Q, Kx, Vx, DEV, causal=causal, scale=scale, variant=variant,
                                                        window=window)
                    if variant == "auto" and layout == "bnhd" and window is None:
                        continue  # (AUTO: the GQA form's table and the MHA table differ on a non-mergeable layout)
                    assert torch.equal(O.view(torch.uint8), Om.view(torch.uint8)), what
                    assert torch.equal(L.view(torch.uint8), Lm.view(torch.uint8)), what


def test_forward_ragged_long_and_large_group():
    for N, H, H_kv, layout, B in ((4100, 16, 2, "contig", 2), (4100, 8, 1, "bnhd", 2), (1000, 32, 4, "bnhd", 3)):
        Q, K, V, Kx, Vx = make(B, H, H_kv, N, 128, B16, layout, N)
        for causal in (False, True):
            O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=0.088)
            check(O, L, *truth(Q, K, V, causal, 0.088, None), B16, (N, H, H_kv, layout, causal))
            Om, Lm = fa.flash_attention_forward(Q, Kx, Vx, DEV, causal=causal, scale=0.088)
            if layout != "bnhd":  # (the non-mergeable view runs the GQA form; AUTO may pick another MHA kernel)
                assert torch.equal(O, Om) and torch.equal(L, Lm)


BWD = [(B16, 128, ("auto", "mfma16", "generic")), (F16, 64, ("mfma16", "generic")), (F32, 64, ("auto", "generic")),
       (F64, 32, ("generic",)), (B16, 40, ("auto",))]


@pytest.mark.parametrize("dtype,d,variants", BWD)
@pytest.mark.parametrize("layout,B", LAYOUTS)
def test_backward_against_truth_bit_identical_dq_deterministic_dkdv(dtype, d, variants, layout, B):
    H = 8
    scale = 1.0 / math.sqrt(d)
    for N in (200, 1000):
        if dtype == F64 and N > 200:
            continue
        for H_kv in (8, 4, 1):
            Q, K, V, Kx, Vx = make(B, H, H_kv, N, d, dtype, layout, 7 * N + H_kv, amp=0.8)
            dO = make(B, H, H, N, d, dtype, "contig", N + 1)[0]
            for causal, window in ((False, None), (True, None), (False, (63, 64))):
                O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale, window=window)
                t = grads_truth(Q, K, V, dO, causal, scale, window)
                for variant in variants:
                    what = (layout, N, H_kv, causal, window, variant)
                    g = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=scale, variant=variant,
                                                    window=window)
                    assert g[1].shape == K.shape and g[2].shape == V.shape, what
                    for name, a, b in zip("QKV", g, t):
                        assert torch.isfinite(a).all(), what
                        err = (a.double() - b).abs().max().item()
                        assert err <= BWD_REL[dtype] * max(1.0, b.abs().max().item()), (what, name, err)
                    g2 = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=scale, variant=variant,
                                                     window=window)
                    assert torch.equal(g[1], g2[1]) and torch.equal(g[2], g2[2]), what
                    gm = fa.flash_attention_backward(Q, Kx, Vx, O, dO, L, DEV, causal=causal, scale=scale, variant=variant,
                                                     window=window)
                    if not (variant == "auto" and dtype == F32):  # (AUTO: the MHA call takes the fp32 matrix kernel)
                        assert torch.equal(g[0], gm[0]), what
                    for a, b in zip(g[1:], gm[1:]):  # the group sum of the MHA gradients, in another order
                        ref = group_sum(b.double(), H_kv)
                        assert (a.double() - ref).abs().max() <= BWD_REL[dtype] * max(1.0, ref.abs().max().item()), what


def test_mfma32_backward_refuses_gqa():
    Q, K, V, _, _ = make(1, 4, 2, 64, 64, F32, "contig", 1)
    O, L = fa.flash_attention_forward(Q, K, V, DEV)
    with pytest.raises(TypeError):
        backward_native(Q, K, V, O, O, L, variant="mfma32")


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.mark.parametrize("dtype,d,variant", [(B16, 128, "a64"), (B16, 128, "auto"), (F16, 64, "mfma16d"), (F32, 64, "generic")])
def test_equal_heads_through_the_new_entry_points_are_the_old_calls(dtype, d, variant):
    N, H = 300, 4
    Q, K, V, _, _ = make(2, H, H, N, d, dtype, "contig", 5)
    dO = make(2, H, H, N, d, dtype, "contig", 6)[0]
    de = convert_triton_dtype(dtype)
    for causal, window in ((False, (-1, -1)), (True, (-1, -1)), (False, (40, 3))):
        O0, L0 = (torch.empty_like(Q), torch.empty(2, H, N, 1, dtype=dtype, device=DEV))
        O1, L1 = torch.empty_like(O0), torch.empty_like(L0)
        args = (_i64(Q.stride()), _i64(K.stride()), _i64(V.stride()), _i64(O0.stride()), _i64(L0.stride()[:2]))
        v = _lib.VARIANTS[variant]
        rc0 = _lib.lib().fa2_fwd_window_variant(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O0.data_ptr(), L0.data_ptr(), *args,
                                                2, H, N, d, de, causal, 0.1, window[0], window[1], None, v)
        rc1 = _lib.lib().fa2_fwd_gqa_variant(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O1.data_ptr(), L1.data_ptr(), *args,
                                             2, H, H, N, d, de, causal, 0.1, window[0], window[1], None, v)
        assert rc0 == rc1
        if rc0 != 0:
            continue
        torch.cuda.synchronize()
        assert torch.equal(O0, O1) and torch.equal(L0, L1)
        grads = []
        for fn, extra in ((_lib.lib().fa2_bwd_window_variant, ()), (_lib.lib().fa2_bwd_gqa_variant, (H,))):
            dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
            D = torch.empty(2 * 2 * H * N, dtype=torch.float32, device=DEV)
            st = [_i64(t.stride()) for t in (Q, K, V, O0, dO, dQ, dK, dV)] + [_i64(L0.stride()[:2])]
            bv = 0 if variant == "auto" else (2 if dtype in (B16, F16) else 1)
            rc = fn(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O0.data_ptr(), dO.data_ptr(), L0.data_ptr(), dQ.data_ptr(),
                    dK.data_ptr(), dV.data_ptr(), D.data_ptr(), *st, 2, H, *extra, N, d, de, causal, 0.1, window[0], window[1],
                    None, bv)
            assert rc == 0
            grads.append((dQ, dK, dV))
        torch.cuda.synchronize()
        for a, b in zip(*grads):
            assert torch.equal(a, b)


SENT = {B16: -3.0, F16: -3.0, F32: -3.0}


@pytest.mark.parametrize("dtype,fvar,bvar,layout", [(B16, "auto", "auto", "contig"), (B16, "mfma16d", "mfma16", "bnhd"),
                                                    (F32, "generic", "generic", "contig"), (F16, "a64d", "generic", "contig")])
def test_canary_arenas(dtype, fvar, bvar, layout):
    B, H, H_kv, N, d = 2, 8, 2, 300, 64 if fvar == "a64d" else 128
    Q, K, V, _, _ = make(B, H, H_kv, N, d, dtype, layout, 11)
    dO = make(B, H, H, N, d, dtype, "contig", 12)[0]

    def arena(h):  # (B, h, N, d) inside a larger buffer: rows before / after, extra columns
        buf = torch.full((B, h, N + 8, d + 16), SENT[dtype], dtype=dtype, device=DEV)
        return buf, buf[:, :, 4:4 + N, 8:8 + d]

    Ob, O = arena(H)
    L = torch.empty(B, H, N, 1, dtype=dtype, device=DEV)
    _lib.fa2_fwd(Q, K, V, O, L, convert_triton_dtype(dtype), causal=True, scale=0.1, variant=_lib.VARIANTS[fvar])
    check(O, L, *truth(Q, K, V, True, 0.1, None), dtype, "canary")
    (dKb, dK), (dVb, dV) = arena(H_kv), arena(H_kv)
    dQ = torch.empty_like(Q)
    D = torch.empty(2 * B * H * N, dtype=torch.float32, device=DEV)
    _lib.fa2_bwd(Q, K, V, O, dO, L, dQ, dK, dV, D, convert_triton_dtype(dtype), causal=True, scale=0.1,
                 variant=_lib.BWD_VARIANTS[bvar])
    torch.cuda.synchronize()
    for buf, view in ((Ob, O), (dKb, dK), (dVb, dV)):
        outside = buf.clone()
        outside[:, :, 4:4 + N, 8:8 + d] = SENT[dtype]
        assert (outside == SENT[dtype]).all()
        assert torch.isfinite(view).all()
    t = grads_truth(Q, K, V, dO, True, 0.1, None)
    for a, b in zip((dQ, dK, dV), t):
        assert (a.double() - b).abs().max() <= BWD_REL[dtype] * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("cls", [FlashAttention, FlashAttentionDeterministic])
def test_autograd_through_apply(cls):
    B, H, H_kv, N, d = 2, 8, 2, 256, 128
    Q, K, V, _, _ = make(B, H, H_kv, N, d, B16, "contig", 21, amp=0.8)
    Q, K, V = (t.detach().requires_grad_() for t in (Q, K, V))
    dO = make(B, H, H, N, d, B16, "contig", 22)[0]
    O = cls.apply(Q, K, V, True, 0.09)
    O.backward(dO)
    assert K.grad.shape == K.shape and V.grad.shape == V.shape
    for a, b in zip((Q.grad, K.grad, V.grad), grads_truth(Q, K, V, dO, True, 0.09, None)):
        assert (a.double() - b).abs().max() <= BWD_REL[B16] * max(1.0, b.abs().max().item())


def test_gradcheck_f64():
    for H, H_kv, causal, window in ((4, 2, False, None), (4, 1, True, None), (6, 3, False, (2, 1))):
        Q = torch.randn(1, H, 9, 16, dtype=torch.float64, device=DEV, requires_grad=True)
        K, V = (torch.randn(1, H_kv, 9, 16, dtype=torch.float64, device=DEV, requires_grad=True) for _ in range(2))
        f = lambda q, k, v: FlashAttention.apply(q, k, v, causal, 0.5, window)  # noqa: E731
        assert torch.autograd.gradcheck(f, (Q, K, V), eps=1e-6, atol=1e-5, rtol=1e-4)


def _cu(lengths):
    return torch.tensor([0] + list(torch.tensor(lengths).cumsum(0).tolist()), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dtype,d,variant", [(B16, 128, "auto"), (F16, 64, "mfma16d"), (B16, 128, "mfma16d_w4"),
                                             (F32, 64, "generic"), (B16, 40, "auto")])
def test_varlen_gqa_against_per_sequence_truth(dtype, d, variant):
    H, H_kv = 8, 2
    lq, lk = [100, 0, 257, 64, 300, 5], [130, 40, 257, 0, 200, 77]  # N_q != N_k both ways, empty sequences
    cu_q, cu_k = _cu(lq), _cu(lk)
    g = torch.Generator().manual_seed(3)
    Q = (torch.randn(sum(lq), H, d, generator=g) * 0.8).to(dtype).to(DEV)
    K, V = ((torch.randn(sum(lk), H_kv, d, generator=g) * 0.8).to(dtype).to(DEV) for _ in range(2))
    dO = (torch.randn(sum(lq), H, d, generator=g) * 0.5).to(dtype).to(DEV)
    bvar = {"generic": "generic", "auto": "auto"}.get(variant, "mfma16")
    for causal, window in ((False, None), (True, None), (False, (50, 20))):
        O, L = varlen_forward(Q, K, V, cu_q, cu_k, max(lq), max(lk), causal=causal, scale=0.1, window=window, variant=variant)
        dQ, dK, dV = varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, max(lq), max(lk), causal=causal, scale=0.1, window=window,
                                     variant=bvar)
        assert dK.shape == K.shape and dV.shape == V.shape
        mask = varlen_mask(cu_q, cu_k, causal, window).to(DEV)
        q = Q.double().requires_grad_()
        kk, vv = (t.double().detach().requires_grad_() for t in (K, V))
        S = torch.einsum("qhd,khd->hqk", q, expand_kv(kk.transpose(0, 1), H).transpose(0, 1)) * f32(0.1)
        S = S.masked_fill(~mask, float("-inf"))
        rows = mask.any(-1)
        P = torch.zeros_like(S)
        P[:, rows] = torch.softmax(S[:, rows], -1)
        Oref = torch.einsum("hqk,khd->qhd", P, expand_kv(vv.transpose(0, 1), H).transpose(0, 1))
        Oref.backward(dO.double())
        assert (O.double() - Oref).abs().max() <= O_TOL[dtype], (causal, window)
        assert (O[~rows] == 0).all() and torch.isinf(L[:, ~rows]).all()
        for a, b in ((dQ, q.grad), (dK, kk.grad), (dV, vv.grad)):
            assert torch.isfinite(a).all()
            assert (a.double() - b).abs().max() <= BWD_REL[dtype] * max(1.0, b.abs().max().item()), (causal, window)
        dK2 = varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, max(lq), max(lk), causal=causal, scale=0.1, window=window,
                              variant=bvar)[1]
        assert torch.equal(dK, dK2)


@pytest.mark.parametrize("dtype,fvar,bvar", [(B16, "mfma16d_w4", "mfma16"), (B16, "mfma16d", "mfma16"),
                                             (F32, "generic", "generic")])
def test_varlen_equal_lengths_equal_dense_gqa(dtype, fvar, bvar):
    B, H, H_kv, N, d = 3, 8, 2, 320, 128 if dtype == B16 else 64
    Q, K, V, _, _ = make(B, H, H_kv, N, d, dtype, "contig", 31)
    dO = make(B, H, H, N, d, dtype, "contig", 32)[0]
    cu = _cu([N] * B)
    pk = lambda t: t.transpose(1, 2).reshape(B * N, t.shape[1], d).contiguous()  # noqa: E731
    for causal, window in ((False, None), (True, None), (False, (70, 9))):
        O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=0.1, variant=fvar, window=window)
        g = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=0.1, variant=bvar, window=window)
        Ov, Lv = varlen_forward(pk(Q), pk(K), pk(V), cu, cu, N, N, causal=causal, scale=0.1, window=window, variant=fvar)
        assert torch.equal(Ov, pk(O))
        assert torch.equal(Lv.view(H, B, N).transpose(0, 1), L.squeeze(-1))
        gv = varlen_backward(pk(Q), pk(K), pk(V), Ov, pk(dO), Lv, cu, cu, N, N, causal=causal, scale=0.1, window=window,
                             variant=bvar)
        for a, b in zip(gv, g):
            assert torch.equal(a, pk(b))


def test_varlen_autograd():
    H, H_kv, d = 4, 1, 64
    lq = [33, 70]
    cu = _cu(lq)
    Q = torch.randn(sum(lq), H, d, dtype=B16, device=DEV, requires_grad=True)
    K, V = (torch.randn(sum(lq), H_kv, d, dtype=B16, device=DEV, requires_grad=True) for _ in range(2))
    O = FlashAttentionVarlen.apply(Q, K, V, cu, cu, max(lq), max(lq), True, 0.125)
    O.float().sum().backward()
    assert K.grad.shape == K.shape and torch.isfinite(K.grad).all() and torch.isfinite(Q.grad).all()


@pytest.mark.parametrize("dtype,d,variant", [(F32, 16, "auto"), (F32, 16, "generic"), (B16, 40, "generic")])
def test_merge_keeps_the_generic_grid_limit(dtype, d, variant):
    # B * H_kv = 131072 merged batches would exceed the generic kernel's grid (y <= 65535): the call must still run, unmerged
    B, H, H_kv, N = 16384, 16, 8, 8
    Q, K, V, Kx, Vx = make(B, H, H_kv, N, d, dtype, "contig", 41)
    O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=True, scale=0.3, variant=variant)
    check(O, L, *truth(Q, K, V, True, 0.3, None), dtype, (dtype, d, variant))
    Om, Lm = fa.flash_attention_forward(Q, Kx, Vx, DEV, causal=True, scale=0.3, variant=variant)
    assert torch.equal(O, Om) and torch.equal(L, Lm)


def test_mqa_merges_whatever_the_size_one_head_stride():
    # (B, N, 1, d).transpose(1, 2) is contiguous for torch with a head stride of d: the MQA problem must still take the merged
    # path, i.e. every dense variant, and equal the MHA call on expanded K / V
    B, H, N, d = 3, 8, 512, 128
    Q = (torch.randn(B, H, N, d, device=DEV) * 0.5).to(B16)
    K, V = ((torch.randn(B, N, 1, d, device=DEV) * 0.5).to(B16).transpose(1, 2) for _ in range(2))
    assert K.is_contiguous() and K.stride(1) != K.stride(0)
    for variant in ("a64", "a16", "mfma16", "auto"):
        for causal in (False, True):
            O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=0.09, variant=variant)
            Om, Lm = fa.flash_attention_forward(Q, K.expand(B, H, N, d).contiguous(), V.expand(B, H, N, d).contiguous(), DEV,
                                                causal=causal, scale=0.09, variant=variant)
            assert torch.equal(O, Om) and torch.equal(L, Lm), (variant, causal)
