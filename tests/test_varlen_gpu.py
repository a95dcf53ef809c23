"""Variable-length (packed) attention on the GPU: forward O and L against the fp64 per-sequence truth, empty rows, bit-identity
with the dense call of the same forced variant, the backward against fp64 autograd through the masked softmax, determinism,
gradcheck, a strided QKV buffer, canary arenas, malformed offsets and one packed tensor above 2 GiB."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import FlashAttentionVarlen, convert_triton_dtype
from oracle import fa2_bwd_arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the bars of tests/test_window_gpu.py
O_TOL = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 5e-2, torch.float64: 1e-6}
BWD_REL = {torch.float16: 4e-3, torch.bfloat16: 2.5e-2, torch.float32: 2e-4, torch.float64: 1e-6}
LQ = [0, 1, 31, 255, 256, 1000, 2065, 300, 40]
LK = [5, 1, 255, 31, 1000, 256, 2065, 0, 97]   # N_q < N_k, N_q > N_k, N_k = 0, N_q = 0
WINDOWS = (None, (64, 0), (100, 50), (-1, 17))


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def cu_of(lengths):
    return torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def band(nq, nk, causal, window):
    """(nq, nk) visible pairs of one sequence: bottom-right aligned (include/fa2_fwd.h; the rule is oracle.fa2_bwd_arith.band)."""
    return fa2_bwd_arith.band(nq, nk, causal, window, DEV)


def varlen_reference(Q, K, V, lq, lk, causal, scale, window, seqs=None):
    """fp64 truth, one sequence at a time (differentiable): O (total_q, H, d), L (H, total_q); rows without a visible key
    get O = 0 and L = +inf."""
    q, k, v = Q.double(), K.double(), V.double()
    cq, ck = [0] + torch.tensor(lq).cumsum(0).tolist(), [0] + torch.tensor(lk).cumsum(0).tolist()
    outs, ls = [], []
    for b in (range(len(lq)) if seqs is None else seqs):
        nq, nk = lq[b], lk[b]
        qs, ks, vs = q[cq[b]:cq[b] + nq], k[ck[b]:ck[b] + nk], v[ck[b]:ck[b] + nk]
        S = torch.einsum("qhd,khd->hqk", qs, ks) * f32(scale)
        m = band(nq, nk, causal, window)
        S = S.masked_fill(~m, float("-inf"))
        vis = m.any(-1)
        P = torch.where(vis.view(1, nq, 1), torch.softmax(S.masked_fill(~vis.view(1, nq, 1), 0.0), -1), 0.0)
        outs.append(torch.einsum("hqk,khd->qhd", P, vs))
        ls.append(torch.where(vis, torch.logsumexp(S, -1) * math.log2(math.e), math.inf))
    return torch.cat(outs), torch.cat(ls, 1)


def packed(lq, lk, H, d, dtype, seed, amp=0.5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, H, d, generator=g) * amp).to(dtype).to(DEV) for n in (sum(lq), sum(lk), sum(lk))]


def ulp(dtype, x):
    mant = {torch.float16: 10, torch.bfloat16: 7}[dtype]
    return 2.0 ** (math.floor(math.log2(max(abs(x), 1e-30))) - mant)


def check_forward(O, L, O_ref, L_ref, dtype, what):
    O, L = O.double(), L.double()
    assert not torch.isnan(O).any() and not torch.isnan(L).any(), what
    empty = torch.isinf(L_ref)
    assert torch.equal(torch.isinf(L), empty) and (L[empty] > 0).all(), what  # exactly the empty rows, +inf
    assert (O.permute(1, 0, 2)[empty] == 0).all(), what
    assert (O - O_ref).abs().max() <= O_TOL[dtype], what
    Lf, Lr = L[~empty], L_ref[~empty]
    if Lr.numel() == 0:
        return
    if dtype in (torch.float32, torch.float64):
        assert ((Lf - Lr).abs() <= 5e-5 * Lr.abs().clamp(min=1)).all(), what
    else:
        assert (Lf - Lr).abs().max() <= 1.01 * ulp(dtype, Lr.abs().max().item()), what


CASES = [(dt, v, d) for dt in (torch.float16, torch.bfloat16) for v in ("auto", "generic", "mfma16d", "mfma16d_w4")
         for d in (64, 128)]
CASES += [(dt, v, 64) for dt in (torch.float32, torch.float64) for v in ("auto", "generic")]
CASES += [(torch.bfloat16, "auto", 40), (torch.float32, "auto", 40)]


@pytest.mark.parametrize("dtype,variant,d", CASES)
def test_forward_against_fp64_truth(dtype, variant, d):
    H = 2
    scale = 1.0 / math.sqrt(d)
    Q, K, V = packed(LQ, LK, H, d, dtype, d)
    cu_q, cu_k = cu_of(LQ), cu_of(LK)
    for causal in (False, True):
        for window in WINDOWS:
            O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, max(LQ), max(LK), DEV, causal=causal, scale=scale,
                                                     window=window, variant=variant)
            O_ref, L_ref = varlen_reference(Q, K, V, LQ, LK, causal, scale, window)
            assert O.shape == Q.shape and L.shape == (H, sum(LQ))
            check_forward(O, L, O_ref, L_ref, dtype, (variant, causal, window))


@pytest.mark.parametrize("variant", ["mfma16d", "mfma16d_w4", "generic"])
def test_equal_lengths_bit_identical_to_dense(variant):
    B, H, N, d = 3, 4, 300, 128
    g = torch.Generator().manual_seed(7)
    Qd, Kd, Vd = ((torch.randn(B, H, N, d, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(3))
    pack = lambda t: t.transpose(1, 2).reshape(B * N, H, d).contiguous()
    Q, K, V = pack(Qd), pack(Kd), pack(Vd)
    cu = cu_of([N] * B)
    for causal, window in ((False, None), (True, None), (False, (50, 10))):
        Od, Ld = fa.flash_attention_forward(Qd, Kd, Vd, DEV, causal=causal, scale=0.09, variant=variant, window=window)
        O, L = fa.flash_attention_varlen_forward(Q, K, V, cu, cu, N, N, DEV, causal=causal, scale=0.09, window=window,
                                                 variant=variant)
        assert torch.equal(O, pack(Od)), (variant, causal, window)
        assert torch.equal(L, Ld.squeeze(-1).permute(1, 0, 2).reshape(H, B * N)), (variant, causal, window)


def test_empty_rows_and_their_gradients():
    lq, lk = [40, 8, 5, 0], [8, 40, 0, 6]  # causal with N_q > N_k: 32 empty rows; N_k = 0: all rows empty
    H, d = 2, 64
    Q, K, V = packed(lq, lk, H, d, torch.bfloat16, 11)
    cu_q, cu_k = cu_of(lq), cu_of(lk)
    for variant in ("auto", "generic", "mfma16d"):
        O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, 40, 40, DEV, causal=True, variant=variant)
        empty = torch.cat([torch.arange(0, 32), torch.arange(48, 53)]).to(DEV)
        assert (O[empty] == 0).all() and torch.isinf(L[:, empty]).all() and (L[:, empty] > 0).all(), variant
        assert not torch.isnan(O).any() and not torch.isnan(L).any()
    dO = torch.randn_like(Q)
    dQ, dK, dV = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, 40, 40, DEV, causal=True)
    assert (dQ[empty] == 0).all()
    for t in (dQ, dK, dV):
        assert not torch.isnan(t).any() and torch.isfinite(t).all()


BWD_CASES = [(dt, d, v) for dt in (torch.float16, torch.bfloat16) for d in (64, 128) for v in ("auto", "generic", "mfma16")]
BWD_CASES += [(torch.float32, 64, "auto"), (torch.float64, 64, "auto"), (torch.bfloat16, 40, "auto")]
BLQ = [0, 1, 31, 255, 256, 300, 64]
BLK = [3, 1, 255, 31, 300, 0, 130]


@pytest.mark.parametrize("dtype,d,variant", BWD_CASES)
def test_backward_against_fp64_autograd(dtype, d, variant):
    H, scale = 2, 1.0 / math.sqrt(d)
    Q, K, V = packed(BLQ, BLK, H, d, dtype, 100 + d)
    dO = packed(BLQ, BLK, H, d, dtype, 200 + d)[0]
    cu_q, cu_k = cu_of(BLQ), cu_of(BLK)
    for causal, window in ((False, None), (True, None), (False, (40, 7)), (True, (-1, 3))):
        O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, max(BLQ), max(BLK), DEV, causal=causal, scale=scale,
                                                 window=window)
        grads = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, max(BLQ), max(BLK), DEV, causal=causal,
                                                   scale=scale, window=window, variant=variant)
        q, k, v = (t.detach().double().clone().requires_grad_() for t in (Q, K, V))  # (fresh leaves: .double() of fp64 is a no-op)
        O_ref, _ = varlen_reference(q, k, v, BLQ, BLK, causal, scale, window)
        O_ref.backward(dO.double())
        for name, a, b in zip("QKV", grads, (q.grad, k.grad, v.grad)):
            assert not torch.isnan(a).any(), name
            err = (a.double() - b).abs().max().item()
            assert err <= BWD_REL[dtype] * max(1.0, b.abs().max().item()), (causal, window, name, err)
        # keys no query sees: exactly zero gradients
        seen = torch.zeros(sum(BLK), dtype=torch.bool, device=DEV)
        cq, ck = [0] + torch.tensor(BLQ).cumsum(0).tolist(), [0] + torch.tensor(BLK).cumsum(0).tolist()
        for b in range(len(BLQ)):
            if BLQ[b] and BLK[b]:
                seen[ck[b]:ck[b] + BLK[b]] = band(BLQ[b], BLK[b], causal, window).any(0)
        assert (grads[1][~seen] == 0).all() and (grads[2][~seen] == 0).all(), (causal, window)
        again = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, max(BLQ), max(BLK), DEV, causal=causal,
                                                   scale=scale, window=window, variant=variant)
        for a, b in zip(grads, again):
            assert torch.equal(a, b)  # deterministic


@pytest.mark.parametrize("variant", ["mfma16", "generic"])
def test_backward_equal_lengths_bit_identical_to_dense(variant):
    B, H, N, d = 3, 4, 300, 128
    g = torch.Generator().manual_seed(8)
    Qd, Kd, Vd, dOd = ((torch.randn(B, H, N, d, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(4))
    pack = lambda t: t.transpose(1, 2).reshape(B * N, H, d).contiguous()
    Q, K, V, dO = pack(Qd), pack(Kd), pack(Vd), pack(dOd)
    cu = cu_of([N] * B)
    for causal, window in ((False, None), (True, None), (False, (50, 10))):
        Od, Ld = fa.flash_attention_forward(Qd, Kd, Vd, DEV, causal=causal, scale=0.09, window=window)
        dense = fa.flash_attention_backward(Qd, Kd, Vd, Od, dOd, Ld, DEV, causal=causal, scale=0.09, variant=variant,
                                            window=window)
        L = Ld.squeeze(-1).permute(1, 0, 2).reshape(H, B * N).contiguous()
        grads = fa.flash_attention_varlen_backward(Q, K, V, pack(Od), dO, L, cu, cu, N, N, DEV, causal=causal, scale=0.09,
                                                   window=window, variant=variant)
        for name, a, b in zip("QKV", grads, dense):
            assert torch.equal(a, pack(b)), (variant, causal, window, name)


def test_backward_auto_runs_the_mfma_kernel_where_it_can():
    # forced generic and AUTO differ in their rounding points: AUTO must not be the VALU kernel for bf16 at d = 128
    Q, K, V = packed([300, 100], [300, 257], 2, 128, torch.bfloat16, 31)
    cu_q, cu_k = cu_of([300, 100]), cu_of([300, 257])
    O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, 300, 300, DEV, causal=True)
    dO = torch.randn_like(Q)
    run = lambda v: fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, 300, 300, DEV, causal=True, variant=v)
    auto, mfma, gen = run("auto"), run("mfma16"), run("generic")
    assert all(torch.equal(a, b) for a, b in zip(auto, mfma))
    assert not all(torch.equal(a, b) for a, b in zip(auto, gen))


def test_gradcheck_f64():
    lq, lk = [3, 5, 0, 4], [5, 3, 2, 4]
    H, d = 1, 16
    Q, K, V = (t.requires_grad_() for t in packed(lq, lk, H, d, torch.float64, 5))
    cu_q, cu_k = cu_of(lq), cu_of(lk)
    for causal, window in ((False, None), (True, None), (False, (1, 1))):
        f = lambda q, k, v: FlashAttentionVarlen.apply(q, k, v, cu_q, cu_k, 5, 5, causal, 0.8, window)
        assert torch.autograd.gradcheck(f, (Q, K, V), eps=1e-6, atol=1e-5, nondet_tol=0.0)


def test_strided_qkv_buffer():
    lq = [100, 257, 33]
    H, d = 4, 128
    g = torch.Generator().manual_seed(9)
    buf = (torch.randn(sum(lq), 3, H, d, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    Q, K, V = buf[:, 0], buf[:, 1], buf[:, 2]
    cu = cu_of(lq)
    for variant in ("auto", "mfma16d", "generic"):
        for causal in (False, True):
            O, L = fa.flash_attention_varlen_forward(Q, K, V, cu, cu, max(lq), max(lq), DEV, causal=causal, scale=0.088,
                                                     variant=variant)
            O_c, L_c = fa.flash_attention_varlen_forward(Q.contiguous(), K.contiguous(), V.contiguous(), cu, cu, max(lq),
                                                         max(lq), DEV, causal=causal, scale=0.088, variant=variant)
            assert torch.equal(O, O_c) and torch.equal(L, L_c), (variant, causal)
            O_ref, L_ref = varlen_reference(Q, K, V, lq, lq, causal, 0.088, None)
            check_forward(O, L, O_ref, L_ref, torch.bfloat16, (variant, causal))
    dO = torch.randn_like(Q)
    grads = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu, cu, max(lq), max(lq), DEV, causal=True, scale=0.088)
    grads_c = fa.flash_attention_varlen_backward(Q.contiguous(), K.contiguous(), V.contiguous(), O, dO, L, cu, cu, max(lq),
                                                 max(lq), DEV, causal=True, scale=0.088)
    for a, b in zip(grads, grads_c):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype,fvar", [(torch.bfloat16, "mfma16d"), (torch.bfloat16, "mfma16d_w4"), (torch.float16, "generic"),
                                        (torch.float32, "generic")])
def test_canary_arenas(dtype, fvar):
    lq, lk = [70, 0, 129, 3], [64, 9, 300, 0]
    H, d, pad = 2, 64, 4096
    Q, K, V = packed(lq, lk, H, d, dtype, 21)
    cu_q, cu_k = cu_of(lq), cu_of(lk)
    tq, tk = sum(lq), sum(lk)
    sentinel = -7.25

    def arena(n):
        a = torch.full((n + 2 * pad,), sentinel, dtype=dtype, device=DEV)
        return a, a[pad:pad + n]

    def untouched(a, n):
        return (a[:pad] == sentinel).all() and (a[pad + n:] == sentinel).all()

    Oa, Ov = arena(tq * H * d)
    La, Lv = arena(H * tq)
    O, L = Ov.view(tq, H, d), Lv.view(H, tq)
    _lib.fa2_fwd_varlen(Q, K, V, O, L, cu_q, cu_k, max(lq), max(lk), convert_triton_dtype(dtype), causal=True, scale=0.125,
                        variant=_lib.VARIANTS[fvar])
    torch.cuda.synchronize()
    assert untouched(Oa, tq * H * d) and untouched(La, H * tq)
    dO = torch.randn_like(Q)
    arenas = [arena(n) for n in (tq * H * d, tk * H * d, tk * H * d)]
    dQ, dK, dV = arenas[0][1].view(tq, H, d), arenas[1][1].view(tk, H, d), arenas[2][1].view(tk, H, d)
    D = torch.empty(2, H, tq, dtype=torch.float64 if dtype == torch.float64 else torch.float32, device=DEV)
    _lib.fa2_bwd_varlen(Q, K, V, O, dO, L, dQ, dK, dV, D, cu_q, cu_k, max(lq), max(lk), convert_triton_dtype(dtype),
                        causal=True, scale=0.125)
    torch.cuda.synchronize()
    for (a, _), n in zip(arenas, (tq * H * d, tk * H * d, tk * H * d)):
        assert untouched(a, n)


def test_malformed_offsets_complete():
    # offsets past total, decreasing and negative: the kernels clamp them (no values asserted -- a bounds check)
    H, d = 2, 128
    Q, K, V = packed([200], [300], H, d, torch.bfloat16, 4)
    cu_q = torch.tensor([0, 150, 10_000, 90, -5, 200], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([-100, 300, 7, 1 << 30, 0, 500], dtype=torch.int32, device=DEV)
    for variant in ("mfma16d", "mfma16d_w4", "generic"):
        for causal in (False, True):
            fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, 256, 512, DEV, causal=causal, variant=variant)
    O, L = fa.flash_attention_varlen_forward(Q, K, V, cu_q, cu_k, 256, 512, DEV)
    fa.flash_attention_varlen_backward(Q, K, V, O, torch.randn_like(Q), L, cu_q, cu_k, 256, 512, DEV, causal=True)
    torch.cuda.synchronize()


def test_large_packed_tensor_takes_the_mfma_path():
    # 600 Ki tokens x H16 x d128 bf16 = 2.4 GiB per tensor: 32-bit offsets span one sequence, so the MFMA kernel still runs
    H, d, n = 16, 128, 4096
    B = 600 * 1024 // n
    lengths = [n] * B
    total = n * B
    Q = torch.empty(total, H, d, dtype=torch.bfloat16, device=DEV)
    K, V = torch.empty_like(Q), torch.empty_like(Q)
    assert Q.numel() * 2 > (1 << 31)
    g = torch.Generator(device=DEV).manual_seed(1)
    for t in (Q, K, V):
        t.normal_(0, 0.5, generator=g)
    cu = cu_of(lengths)
    O, L = fa.flash_attention_varlen_forward(Q, K, V, cu, cu, n, n, DEV, causal=True, scale=0.088, variant="mfma16d")
    torch.cuda.synchronize()
    for b in (B - 2, B - 1):
        sl = slice(b * n, b * n + n)
        O_ref, L_ref = varlen_reference(Q[sl, :2], K[sl, :2], V[sl, :2], [n], [n], True, 0.088, None)
        check_forward(O[sl, :2], L[:2, sl], O_ref, L_ref, torch.bfloat16, b)
