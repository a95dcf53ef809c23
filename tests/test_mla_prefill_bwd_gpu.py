"""The packed backward with a value head size of its own (flash_attention_mla_prefill_backward, fa2_bwd_varlen_dv) on the GPU: every
variant and H_kv against fp64 per-sequence autograd under the bars of tests/test_varlen_gpu.py, the matrix kernel against the VALU
kernel, bit-identity with flash_attention_varlen_backward at d_v == d, fused strided buffers on the input and on the output side,
canary arenas, tokens outside every sequence, empty rows, malformed offsets, determinism, linearity in dO, the autograd class,
gradcheck, and which kernel AUTO runs."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_prefill_bwd_cases as C
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import FlashAttentionMLAPrefill, convert_triton_dtype
from oracle import fa2_bwd_arith as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F16, F32, F64 = C.BF16, C.F16, C.F32, C.F64
LQ, LK, H, SCALE = C.LQ, C.LK, C.H, C.SCALE


def cu_of(lengths):
    return torch.tensor(C.starts(lengths), dtype=torch.int32, device=DEV)


def forward(Q, K, V, causal, window, lq=LQ, lk=LK, scale=SCALE):
    return fa.flash_attention_mla_prefill_forward(Q, K, V, cu_of(lq), cu_of(lk), max(lq), max(lk), DEV, causal=causal, scale=scale,
                                                  window=window)


def backward(Q, K, V, O, dO, L, causal, window, variant, lq=LQ, lk=LK, scale=SCALE):
    return fa.flash_attention_mla_prefill_backward(Q, K, V, O, dO, L, cu_of(lq), cu_of(lk), max(lq), max(lk), DEV, causal=causal,
                                                   scale=scale, window=window, variant=variant)


@functools.lru_cache(maxsize=None)
def problem(dtype, h_kv, d, d_v, causal, window):
    """Q, K, V, O, L, dO on the device and the fp64 truth of the gradients, computed once and shared"""
    Q, K, V, dO = (t.to(DEV) for t in C.data(dtype, h_kv, d, d_v))
    O, L = forward(Q, K, V, causal, window)
    return (Q, K, V, O, L, dO), C.truth(Q, K, V, dO, LQ, LK, causal, SCALE, window)


CASES = [(dt, v, 192, 128) for dt in (F16, BF16) for v in ("auto", "mfma16dv", "generic")]
CASES += [(F32, "generic", 192, 128), (F32, "auto", 192, 128), (BF16, "generic", 128, 64), (F32, "generic", 128, 64), (BF16, "generic", 40, 72),
          (F32, "auto", 40, 72), (F64, "generic", 40, 72)]


@pytest.mark.parametrize("h_kv", (4, 2, 1))
@pytest.mark.parametrize("dtype,variant,d,d_v", CASES)
def test_backward_against_fp64_autograd(dtype, variant, d, d_v, h_kv):
    cq, ck = C.starts(LQ), C.starts(LK)
    for causal, window in C.MASKS:
        (Q, K, V, O, L, dO), ref = problem(dtype, h_kv, d, d_v, causal, window)
        got = backward(Q, K, V, O, dO, L, causal, window, variant)
        assert got[0].shape == Q.shape and got[1].shape == K.shape and got[2].shape == V.shape
        missed = C.within_truth(got, ref, dtype)
        assert not missed, (variant, causal, window, missed)
        for b, (nq, nk) in enumerate(zip(LQ, LK)):                       # keys no query sees, queries that see no key: exactly zero
            keep = A.band(nq, nk, causal, window, DEV)
            unseen = ~keep.any(0) if nq else torch.ones(nk, dtype=torch.bool, device=DEV)
            assert (got[1][ck[b]:ck[b] + nk][unseen] == 0).all() and (got[2][ck[b]:ck[b] + nk][unseen] == 0).all(), (causal, window, b)
            blind = ~keep.any(1) if nk else torch.ones(nq, dtype=torch.bool, device=DEV)
            assert (got[0][cq[b]:cq[b] + nq][blind] == 0).all(), (causal, window, b)


@pytest.mark.parametrize("dtype", (F16, BF16))
@pytest.mark.parametrize("h_kv", (4, 2, 1))
def test_matrix_kernel_agrees_with_the_valu_kernel(dtype, h_kv):
    for causal, window in C.MASKS:
        (Q, K, V, O, L, dO), ref = problem(dtype, h_kv, 192, 128, causal, window)
        m, g = (backward(Q, K, V, O, dO, L, causal, window, v) for v in ("mfma16dv", "generic"))
        assert not C.within_truth(m, tuple(t.double() for t in g), dtype, factor=2.0), (causal, window)   # both within the bar of the truth


def test_auto_runs_the_matrix_kernel_at_192_128_and_two_runs_are_bitwise_equal():
    (Q, K, V, O, L, dO), _ = problem(BF16, 2, 192, 128, True, None)
    auto, forced, again, gen = (backward(Q, K, V, O, dO, L, True, None, v) for v in ("auto", "mfma16dv", "mfma16dv", "generic"))
    assert all(torch.equal(a, b) for a, b in zip(auto, forced)) and all(torch.equal(a, b) for a, b in zip(forced, again))
    assert not all(torch.equal(a, b) for a, b in zip(auto, gen))         # (other rounding points: not the VALU kernel)
    assert all(torch.equal(a, b) for a, b in zip(gen, backward(Q, K, V, O, dO, L, True, None, "generic")))
    (Q, K, V, O, L, dO), _ = problem(F32, 2, 192, 128, True, None)       # what it cannot take runs the VALU kernel as it is
    assert all(torch.equal(a, b) for a, b in zip(backward(Q, K, V, O, dO, L, True, None, "auto"), backward(Q, K, V, O, dO, L, True, None, "generic")))


@pytest.mark.parametrize("h_kv", (4, 1))
def test_equal_widths_are_the_varlen_backward_bit_for_bit(h_kv):
    B, N, d = 3, 300, 128
    g = torch.Generator().manual_seed(7)
    Q, K, V, dO = ((torch.randn(B * N, h, d, generator=g) * 0.5).to(BF16).to(DEV) for h in (H, h_kv, h_kv, H))
    cu = cu_of([N] * B)
    for causal, window in ((False, None), (True, None), (False, (50, 10))):
        O, L = fa.flash_attention_varlen_forward(Q, K, V, cu, cu, N, N, DEV, causal=causal, scale=0.09, window=window)
        for variant in ("generic", "auto"):
            got = fa.flash_attention_mla_prefill_backward(Q, K, V, O, dO, L, cu, cu, N, N, DEV, causal=causal, scale=0.09, window=window,
                                                          variant=variant)
            ref = fa.flash_attention_varlen_backward(Q, K, V, O, dO, L, cu, cu, N, N, DEV, causal=causal, scale=0.09, window=window,
                                                     variant=variant)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), (variant, causal, window)


def raw(Q, K, V, O, dO, L, dQ, dK, dV, D, lq, lk, causal, variant, cu_q=None, cu_k=None, max_q=None, max_k=None):
    _lib.fa2_bwd_varlen_dv(Q, K, V, O, dO, L, dQ, dK, dV, D, cu_of(lq) if cu_q is None else cu_q, cu_of(lk) if cu_k is None else cu_k,
                           max(lq) if max_q is None else max_q, max(lk) if max_k is None else max_k, convert_triton_dtype(Q.dtype),
                           causal=causal, scale=SCALE, variant=_lib.BWD_VARLEN_DV_VARIANTS[variant])
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", ("auto", "mfma16dv", "generic"))
def test_fused_buffers_as_two_views_on_either_side(variant):
    h_kv, sentinel = 2, -7.25
    (Q, K, V, O, L, dO), _ = problem(BF16, h_kv, 192, 128, True, None)
    want = backward(Q, K, V, O, dO, L, True, None, variant)
    buf = torch.cat([K, V], -1)                                          # the up-projection's output, K | V per head
    Kv, Vv = buf[..., :192], buf[..., 192:]
    assert not Kv.is_contiguous() and not Vv.is_contiguous()
    got = backward(Q, Kv, Vv, O, dO, L, True, None, variant)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # ... and dK | dV written into the two views of one fused gradient buffer (through the library: the wrapper allocates its own)
    gbuf = torch.full((sum(LK), h_kv, 320), sentinel, dtype=BF16, device=DEV)
    dQ = torch.empty_like(Q)
    D = torch.empty(2, H, sum(LQ), dtype=F32, device=DEV)
    raw(Q, Kv, Vv, O, dO, L, dQ, gbuf[..., :192], gbuf[..., 192:], D, LQ, LK, True, variant)
    assert torch.equal(dQ, want[0]) and torch.equal(gbuf[..., :192], want[1]) and torch.equal(gbuf[..., 192:], want[2])
    # a dK view with room behind it: the row's other columns stay untouched
    wide = torch.full((sum(LK), h_kv, 328), sentinel, dtype=BF16, device=DEV)
    raw(Q, Kv, Vv, O, dO, L, dQ, wide[..., :192], wide[..., 192:320], D, LQ, LK, True, variant)
    assert torch.equal(wide[..., :192], want[1]) and torch.equal(wide[..., 192:320], want[2]) and (wide[..., 320:] == sentinel).all()


@pytest.mark.parametrize("dtype,variant", [(BF16, "mfma16dv"), (F16, "mfma16dv"), (BF16, "auto"), (F16, "generic"), (F32, "generic")])
def test_canary_arenas_unwritten_tokens_and_malformed_offsets(dtype, variant):
    lq, lk = [70, 0, 129, 3], [64, 9, 300, 0]
    h_kv, d, d_v, pad, spare, sentinel = 2, 192, 128, 4096, 5, -7.25
    g = torch.Generator().manual_seed(21)
    tq, tk = sum(lq) + spare, sum(lk) + spare                            # `spare` tokens behind the last sequence belong to none
    Q, K, V, dO = ((torch.randn(n, h, c, generator=g) * 0.5).to(dtype).to(DEV)
                   for n, h, c in ((tq, H, d), (tk, h_kv, d), (tk, h_kv, d_v), (tq, H, d_v)))

    def arena(n, dt=dtype):
        a = torch.full((n + 2 * pad,), sentinel, dtype=dt, device=DEV)
        return a, a[pad:pad + n]

    arenas = [arena(tq * H * d), arena(tk * h_kv * d), arena(tk * h_kv * d_v), arena(2 * H * tq, F32)]
    dQ, dK, dV = arenas[0][1].view(tq, H, d), arenas[1][1].view(tk, h_kv, d), arenas[2][1].view(tk, h_kv, d_v)
    D = arenas[3][1].view(2, H, tq)

    def intact():
        return all((a[:pad] == sentinel).all() and (a[pad + v.numel():] == sentinel).all() for a, v in arenas)

    for causal in (True, False):
        for _, v in arenas:
            v.fill_(sentinel)
        O, L = fa.flash_attention_mla_prefill_forward(Q, K, V, cu_of(lq), cu_of(lk), max(lq), max(lk), DEV, causal=causal, scale=SCALE)
        O[sum(lq):] = 0                                                  # (the forward leaves these unwritten)
        raw(Q, K, V, O, dO, L, dQ, dK, dV, D, lq, lk, causal, variant)
        assert intact(), causal
        assert (dQ[sum(lq):] == sentinel).all() and (dK[sum(lk):] == sentinel).all() and (dV[sum(lk):] == sentinel).all()
        assert (dQ[:sum(lq)] != sentinel).any(-1).all() and (dK[:sum(lk)] != sentinel).any(-1).all()
        got = (dQ[:sum(lq)], dK[:sum(lk)], dV[:sum(lk)])
        assert not any(torch.isnan(t).any() for t in got)
        assert (dQ[70 + 129:70 + 129 + 3] == 0).all()                    # the sequence without keys: dQ rows of 0
        assert (dK[64:73] == 0).all() and (dV[64:73] == 0).all()         # the sequence without queries
        ref = C.truth(Q[:sum(lq)], K[:sum(lk)], V[:sum(lk)], dO[:sum(lq)], lq, lk, causal, SCALE, None)
        assert not C.within_truth(got, ref, dtype), (variant, causal)
    # gaps between sequences, then offsets past total, decreasing and negative: clamped, nothing outside the arenas
    for _, v in arenas:
        v.fill_(sentinel)
    gap_q = torch.tensor([0, 60, 70, 199, 202], dtype=torch.int32, device=DEV)   # max_seqlen_q 50: tokens 50..59 belong to no sequence
    raw(Q, K, V, O, dO, L, dQ, dK, dV, D, lq, lk, False, variant, cu_q=gap_q, max_q=50)
    assert intact() and (dQ[50:60] == sentinel).all() and (dQ[:50] != sentinel).any(-1).all()
    cu_q = torch.tensor([0, 150, 10_000, 90, -5], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([-100, 300, 7, 1 << 30, 0], dtype=torch.int32, device=DEV)
    for causal in (False, True):
        raw(Q, K, V, O, dO, L, dQ, dK, dV, D, lq, lk, causal, variant, cu_q=cu_q, cu_k=cu_k, max_q=256, max_k=512)
        assert intact(), causal


def test_exact_linearity_in_dO_and_zero():
    (Q, K, V, O, L, dO), _ = problem(BF16, 2, 192, 128, True, (100, 50))
    for variant in ("mfma16dv", "generic"):
        one, four = backward(Q, K, V, O, dO, L, True, (100, 50), variant), backward(Q, K, V, O, dO * 4, L, True, (100, 50), variant)
        tiny = torch.finfo(BF16).tiny
        for a, b in zip(one, four):                                      # a power of two moves no rounding point (off the subnormals)
            normal = a.abs().float() >= 8 * tiny
            assert torch.equal((a.float() * 4)[normal], b.float()[normal]), variant
        zero = backward(Q, K, V, O, torch.zeros_like(dO), L, True, (100, 50), variant)
        assert all((t == 0).all() for t in zero), variant


@pytest.mark.parametrize("h_kv", (4, 1))
def test_autograd_class_equals_the_direct_call(h_kv):
    (Q, K, V, O, L, dO), _ = problem(BF16, h_kv, 192, 128, True, (64, 0))
    q, k, v = (t.detach().clone().requires_grad_() for t in (Q, K, V))
    out = FlashAttentionMLAPrefill.apply(q, k, v, cu_of(LQ), cu_of(LK), max(LQ), max(LK), True, SCALE, (64, 0))
    assert torch.equal(out, O)
    out.backward(dO)
    want = backward(Q, K, V, O, dO, L, True, (64, 0), "auto")
    assert all(torch.equal(a, b) for a, b in zip((q.grad, k.grad, v.grad), want))
    q.grad = k.grad = v.grad = None                                      # a dO with a last stride of 2 is made contiguous
    out = FlashAttentionMLAPrefill.apply(q, k, v, cu_of(LQ), cu_of(LK), max(LQ), max(LK), True, SCALE, (64, 0))
    wide = torch.zeros(*dO.shape[:2], 256, dtype=BF16, device=DEV)
    wide[..., ::2] = dO
    out.backward(wide[..., ::2])
    assert all(torch.equal(a, b) for a, b in zip((q.grad, k.grad, v.grad), want))


def test_gradcheck_f64():
    lq, lk = [3, 5], [4, 5]
    g = torch.Generator().manual_seed(3)
    Q, K, V = (torch.randn(n, h, c, generator=g, dtype=F64).to(DEV).requires_grad_() for n, h, c in ((8, 2, 8), (9, 1, 8), (9, 1, 4)))
    for causal, window in ((False, None), (True, None), (False, (2, 1))):
        fn = lambda q, k, v: FlashAttentionMLAPrefill.apply(q, k, v, cu_of(lq), cu_of(lk), 5, 5, causal, 0.4, window)
        assert torch.autograd.gradcheck(fn, (Q, K, V), eps=1e-6, atol=1e-6, rtol=1e-5)
