"""The packed forward with a value head size of its own (flash_attention_mla_prefill_forward, fa2_fwd_varlen_dv) on the GPU: random
data against the fp64 per-sequence truth under the bars of tests/test_varlen_gpu.py, the matrix kernel against the VALU kernel,
bit-identity with fa2_fwd_varlen_gqa_variant(GENERIC) at d_v == d, the fused strided KV buffer as two views, canary arenas around O
and L, malformed offsets, and which kernel AUTO runs."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_varlen_gpu import O_TOL, check_forward, cu_of, varlen_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
LQ = [0, 1, 31, 127, 128, 129, 300, 40]
LK = [5, 1, 65, 31, 128, 257, 300, 0]   # N_q < N_k, N_q > N_k, N_k = 0, N_q = 0
H = 4
WINDOWS = (None, (64, 0), (100, 50), (-1, 17))
SCALE = 1.0 / math.sqrt(192)
MASKS = [(causal, w) for causal in (False, True) for w in WINDOWS]


@functools.lru_cache(maxsize=None)
def data(h_kv, d, d_v, dtype):
    g = torch.Generator().manual_seed(1000 * d + d_v + h_kv)
    return tuple((torch.randn(n, h, c, generator=g) * 0.5).to(dtype).to(DEV)
                 for n, h, c in ((sum(LQ), H, d), (sum(LK), h_kv, d), (sum(LK), h_kv, d_v)))


@functools.lru_cache(maxsize=None)
def reference(h_kv, d, d_v, dtype, causal, window):
    """the fp64 truth of data(...), computed once and shared (query head h reads KV head h // g)"""
    Q, K, V = data(h_kv, d, d_v, dtype)
    g = H // h_kv
    return varlen_reference(Q, K.repeat_interleave(g, 1), V.repeat_interleave(g, 1), LQ, LK, causal, SCALE, window)


def run(Q, K, V, causal, window, variant, lq=LQ, lk=LK):
    return fa.flash_attention_mla_prefill_forward(Q, K, V, cu_of(lq), cu_of(lk), max(lq), max(lk), DEV, causal=causal, scale=SCALE,
                                                  window=window, variant=variant)


CASES = [(dt, v, 192, 128) for dt in (F16, BF16) for v in ("auto", "mfma16dv", "generic")]
CASES += [(dt, "generic", 192, 128) for dt in (F32, F64)]
CASES += [(dt, "generic", d, d_v) for dt in (BF16, F32) for d, d_v in ((128, 64), (40, 72))] + [(F16, "auto", 128, 64), (F64, "auto", 40, 72)]


@pytest.mark.parametrize("h_kv", (4, 2, 1))
@pytest.mark.parametrize("dtype,variant,d,d_v", CASES)
def test_forward_against_fp64_truth(dtype, variant, d, d_v, h_kv):
    Q, K, V = data(h_kv, d, d_v, dtype)
    for causal, window in MASKS:
        O, L = run(Q, K, V, causal, window, variant)
        assert O.shape == (sum(LQ), H, d_v) and O.is_contiguous() and L.shape == (H, sum(LQ))
        check_forward(O, L, *reference(h_kv, d, d_v, dtype, causal, window), dtype, (variant, causal, window))


def test_d_above_512_is_refused():
    Q, K, V = (torch.zeros(8, 1, c, dtype=BF16, device=DEV) for c in (576, 576, 512))
    with pytest.raises(TypeError, match=r"d=576 must be in \[1, 512\]"):
        run(Q, K, V, False, None, "generic", [8], [8])
    with pytest.raises(ValueError, match="d_v"):
        run(Q[..., :192], K[..., :192], torch.zeros(8, 1, 513, dtype=BF16, device=DEV), False, None, "generic", [8], [8])
    with pytest.raises(TypeError, match="mfma16dv kernel"):
        run(Q[..., :128], K[..., :128], V[..., :128], False, None, "mfma16dv", [8], [8])


@pytest.mark.parametrize("dtype", (F16, BF16))
@pytest.mark.parametrize("h_kv", (4, 2, 1))
def test_matrix_kernel_agrees_with_the_valu_kernel(dtype, h_kv):
    Q, K, V = data(h_kv, 192, 128, dtype)
    for causal, window in MASKS:
        (O, L), (Og, Lg) = run(Q, K, V, causal, window, "mfma16dv"), run(Q, K, V, causal, window, "generic")
        assert torch.equal(torch.isinf(L), torch.isinf(Lg))
        assert (O.double() - Og.double()).abs().max() <= 2 * O_TOL[dtype], (causal, window)   # both within the bar of the truth


def test_auto_runs_the_matrix_kernel_at_192_128():
    # forced generic and AUTO differ in their rounding points: AUTO must be the matrix kernel for bf16 at 192 / 128, bit for bit
    Q, K, V = data(2, 192, 128, BF16)
    auto, forced, gen = (run(Q, K, V, True, None, v) for v in ("auto", "mfma16dv", "generic"))
    assert torch.equal(auto[0], forced[0]) and torch.equal(auto[1], forced[1])
    assert not torch.equal(auto[0], gen[0])
    Qf, Kf, Vf = (t.float() for t in (Q, K, V))                        # ... and what it cannot take runs the VALU kernel as it is
    assert all(torch.equal(a, b) for a, b in zip(run(Qf, Kf, Vf, True, None, "auto"), run(Qf, Kf, Vf, True, None, "generic")))


@pytest.mark.parametrize("h_kv", (4, 1))
def test_equal_widths_are_the_varlen_gqa_call_bit_for_bit(h_kv):
    B, N, d = 3, 300, 128
    g = torch.Generator().manual_seed(7)
    Q, K, V = ((torch.randn(B * N, h, d, generator=g) * 0.5).to(BF16).to(DEV) for h in (H, h_kv, h_kv))
    cu = cu_of([N] * B)
    for causal, window in ((False, None), (True, None), (False, (50, 10))):
        for variant in ("generic", "auto"):
            O, L = fa.flash_attention_mla_prefill_forward(Q, K, V, cu, cu, N, N, DEV, causal=causal, scale=0.09, window=window,
                                                          variant=variant)
            Ov, Lv = fa.flash_attention_varlen_forward(Q, K, V, cu, cu, N, N, DEV, causal=causal, scale=0.09, window=window,
                                                       variant=variant)
            assert torch.equal(O, Ov) and torch.equal(L, Lv), (variant, causal, window)


@pytest.mark.parametrize("variant", ("auto", "mfma16dv", "generic"))
def test_fused_kv_buffer_as_two_views(variant):
    h_kv = 2
    g = torch.Generator().manual_seed(9)
    Q = data(h_kv, 192, 128, BF16)[0]
    buf = (torch.randn(sum(LK), h_kv, 192 + 128, generator=g) * 0.5).to(BF16).to(DEV)   # the up-projection's output, K | V per head
    K, V = buf[..., :192], buf[..., 192:]
    assert not K.is_contiguous() and not V.is_contiguous()
    for causal in (False, True):
        O, L = run(Q, K, V, causal, None, variant)
        Oc, Lc = run(Q, K.contiguous(), V.contiguous(), causal, None, variant)
        assert torch.equal(O, Oc) and torch.equal(L, Lc), (variant, causal)
    Qs = torch.zeros(sum(LQ), H, 200, dtype=BF16, device=DEV)
    Qs[..., :192] = Q
    O2, L2 = run(Qs[..., :192], K, V, True, None, variant)             # a strided Q as well
    assert torch.equal(O2, O) and torch.equal(L2, L)


@pytest.mark.parametrize("dtype,variant", [(BF16, "mfma16dv"), (F16, "mfma16dv"), (BF16, "auto"), (F16, "generic"), (F32, "generic")])
def test_canary_arenas_and_unwritten_tokens(dtype, variant):
    lq, lk = [70, 0, 129, 3], [64, 9, 300, 0]
    h_kv, d, d_v, pad, spare = 2, 192, 128, 4096, 5
    g = torch.Generator().manual_seed(21)
    tq, tk = sum(lq) + spare, sum(lk) + spare                          # `spare` tokens behind the last sequence belong to none
    Q, K, V = ((torch.randn(n, h, c, generator=g) * 0.5).to(dtype).to(DEV) for n, h, c in ((tq, H, d), (tk, h_kv, d), (tk, h_kv, d_v)))
    sentinel = -7.25

    def arena(n):
        a = torch.full((n + 2 * pad,), sentinel, dtype=dtype, device=DEV)
        return a, a[pad:pad + n]

    Oa, Ov = arena(tq * H * d_v)                                       # O's token stride is H * d_v: 192 columns written would cross it
    La, Lv = arena(H * tq)
    O, L = Ov.view(tq, H, d_v), Lv.view(H, tq)
    for causal in (True, False):
        Ov.fill_(sentinel)
        Lv.fill_(sentinel)
        _lib.fa2_fwd_varlen_dv(Q, K, V, O, L, cu_of(lq), cu_of(lk), max(lq), max(lk), convert_triton_dtype(dtype), causal=causal,
                               scale=SCALE, variant=_lib.VARLEN_DV_VARIANTS[variant])
        torch.cuda.synchronize()
        for a, n in ((Oa, tq * H * d_v), (La, H * tq)):
            assert (a[:pad] == sentinel).all() and (a[pad + n:] == sentinel).all(), causal
        assert (O[sum(lq):] == sentinel).all() and (L[:, sum(lq):] == sentinel).all()     # tokens outside every sequence
        assert (O[:sum(lq)] != sentinel).any(-1).all() and (L[:, :sum(lq)] != sentinel).all()
        g64 = H // h_kv
        O_ref, L_ref = varlen_reference(Q[:sum(lq)], K[:sum(lk)].repeat_interleave(g64, 1), V[:sum(lk)].repeat_interleave(g64, 1), lq, lk,
                                        causal, SCALE, None)
        check_forward(O[:sum(lq)], L[:, :sum(lq)], O_ref, L_ref, dtype, (variant, causal))


def test_malformed_offsets_complete():
    # the inputs of tests/test_varlen_gpu.py's test: offsets past total, decreasing and negative are clamped (a bounds check)
    Q, K, V = ((torch.randn(n, 2, c) * 0.5).to(BF16).to(DEV) for n, c in ((200, 192), (300, 192), (300, 128)))
    cu_q = torch.tensor([0, 150, 10_000, 90, -5, 200], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([-100, 300, 7, 1 << 30, 0, 500], dtype=torch.int32, device=DEV)
    for variant in ("mfma16dv", "auto", "generic"):
        for causal in (False, True):
            O, L = fa.flash_attention_mla_prefill_forward(Q, K, V, cu_q, cu_k, 256, 512, DEV, causal=causal, variant=variant)
    torch.cuda.synchronize()
    assert O.shape == (200, 2, 128)
