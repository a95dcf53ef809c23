"""fp8 KV-cache decode (fa2_fwd_kvcache_fp8) on the GPU.  Truth is the fp64 reference of tests/test_decode_gpu.py on the
DEQUANTISED cache descale * K8.double(); the bars are that file's own (O_TOL, L within 1.01 ulp): the kernels' arithmetic on the
staged values is the 16-bit kernels' on an exactly representable cache.  Also: the generic-only ground, descale broadcasting,
bit-identity with the 16-bit path at descale 1 (only staging changed), stale rows filled with the formats' NaN / inf bytes, and
the pins carried over from the 16-bit decode (empty rows, workspace poison, determinism, canaries, layouts, rejections)."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import CONFIGS, DEV, LENS, S_K, arena, canaries_intact, check_forward, lens_of, make, reference

pytestmark = pytest.mark.gpu
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
F16, BF16 = torch.float16, torch.bfloat16
POISON = (0x7F, 0xFF, 0x7C, 0xFC)  # e4m3fn: NaN, NaN, 352, -352; e5m2: NaN, NaN, +inf, -inf


def quantized(B, H, H_kv, N_q, S_k, d, dtype, fmt, seed):
    """Q and an fp8 cache by the documented route: make(...) at amp 0.5, then quantize_kv_cache -> per-(b, h_kv) descales."""
    Q, K, V = make(B, H, H_kv, N_q, S_k, d, dtype, seed)
    K8, kd = fa.quantize_kv_cache(K, fmt)
    V8, vd = fa.quantize_kv_cache(V, fmt)
    return Q, K8, V8, kd, vd


def truth(Q, K8, V8, kd, vd, lens, causal, scale, window):
    ones = torch.ones(K8.shape[:2], device=DEV)
    Kd = K8.float().double() * (ones if kd is None else kd.expand_as(ones)).double()[:, :, None, None]
    Vd = V8.float().double() * (ones if vd is None else vd.expand_as(ones)).double()[:, :, None, None]
    return reference(Q, Kd, Vd, lens, causal, scale, window)


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@functools.lru_cache(maxsize=None)
def truth_case(dtype, fmt, d, g, N_q, causal, window, H_kv=2):
    """Inputs and fp64 truth of one CONFIGS entry: computed once, shared by the three variants, never modified."""
    Q, K8, V8, kd, vd = quantized(len(LENS), g * H_kv, H_kv, N_q, S_K, d, dtype, fmt, 7 * d + g + N_q)
    return Q, K8, V8, kd, vd, truth(Q, K8, V8, kd, vd, LENS, causal, 1.0 / math.sqrt(d), window)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("variant", ["auto", "generic", "mfma16"])
@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_forward_against_fp64_truth(dtype, fmt, variant, d):
    lens = lens_of(LENS)
    for g, N_q, causal, window, n in CONFIGS:
        Q, K8, V8, kd, vd, (O_ref, L_ref) = truth_case(dtype, fmt, d, g, N_q, causal, window)
        assert kd.shape == (len(LENS), 2) and len(set(kd.flatten().tolist())) > 1  # non-uniform, not powers of two
        assert not any(math.log2(x).is_integer() for x in kd.flatten().tolist() + vd.flatten().tolist())
        O, L = fa.flash_attention_kvcache_forward(Q, K8, V8, lens, DEV, causal=causal, scale=1.0 / math.sqrt(d), window=window,
                                                  num_splits=n, variant=variant, k_descale=kd, v_descale=vd)
        assert O.shape == Q.shape and L.shape == Q.shape[:3] and O.dtype == dtype and L.dtype == dtype
        check_forward(O, L, O_ref, L_ref, dtype, (dtype, fmt, variant, d, g, N_q, causal, window, n))


def strided_copy(K8, kind):
    """The same fp8 values behind strides the matrix form cannot take."""
    B, H, S, d = K8.shape
    raw = K8.view(torch.uint8)
    if kind == "d_stride":  # element stride 2 over d
        big = torch.full((B, H, S, 2 * d), 0x7F, dtype=torch.uint8, device=DEV)
        big[..., ::2] = raw
        out = big.view(K8.dtype)[..., ::2]
        assert out.stride(3) == 2
    else:                   # rows d + 8 elements apart: not a multiple of 16
        big = torch.full((B, H, S, d + 8), 0x7F, dtype=torch.uint8, device=DEV)
        big[..., :d] = raw
        out = big.view(K8.dtype)[..., :d]
        assert out.stride(2) % 16 == 8
    assert torch.equal(out.view(torch.uint8), raw)
    return out


@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("what", ["d40", "d256", "d_stride", "row_stride", "rows80"])
def test_generic_only_ground(fmt, what):
    lens, H_kv, S_k = [0, 65, 300, 1000], 2, 1000
    d = {"d40": 40, "d256": 256}.get(what, 64)
    g, N_q = (8, 10) if what == "rows80" else (2, 3)
    dtype = BF16 if fmt == E4 else F16
    Q, K8, V8, kd, vd = quantized(len(lens), g * H_kv, H_kv, N_q, S_k, d, dtype, fmt, d + g)
    refs = {}
    Kx, Vx = (strided_copy(K8, what), strided_copy(V8, what)) if what in ("d_stride", "row_stride") else (K8, V8)
    with pytest.raises(TypeError, match="mfma16"):
        fa.flash_attention_kvcache_forward(Q, Kx, Vx, lens_of(lens), DEV, variant="mfma16", k_descale=kd, v_descale=vd)
    for n, causal, window in ((1, True, None), (3, False, (100, 50)), (0, False, None)):
        for variant in ("auto", "generic"):
            O, L = fa.flash_attention_kvcache_forward(Q, Kx, Vx, lens_of(lens), DEV, causal=causal, scale=d ** -0.5, window=window,
                                                      num_splits=n, variant=variant, k_descale=kd, v_descale=vd)
            if (causal, window) not in refs:
                refs[causal, window] = truth(Q, K8, V8, kd, vd, lens, causal, d ** -0.5, window)
            check_forward(O, L, *refs[causal, window], dtype, (fmt, what, variant, n, causal, window))


@pytest.mark.parametrize("variant", ["mfma16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5])
def test_descale_broadcasting(fmt, variant):
    B, H, H_kv, N_q, S_k, d = 3, 8, 2, 2, 600, 64
    Q, K8, V8, kd, vd = quantized(B, H, H_kv, N_q, S_k, d, BF16, fmt, 17)
    lens = lens_of([600, 129, 5])
    full = lambda t: torch.broadcast_to(t, (B, H_kv)).contiguous()
    col = kd[:, :1].contiguous()                                   # (B, 1)
    scalar = torch.tensor(0.37, device=DEV)                        # 0-d
    transposed = kd.t().contiguous().t()                           # (B, H_kv) with strides (1, B)
    assert transposed.stride() == (1, B)
    pairs = [((None, None), (torch.ones(B, H_kv, device=DEV),) * 2),
             ((scalar, scalar), (full(scalar), full(scalar))),
             ((torch.ones(1, 1, device=DEV) * 1.7, vd), (full(torch.tensor(1.7, device=DEV)), vd)),
             ((col, vd[:, :1]), (full(col), full(vd[:, :1]))),
             ((transposed, vd), (kd, vd)),
             ((kd, None), (kd, torch.ones(B, H_kv, device=DEV))),  # K and V descales are independent
             ((None, vd), (torch.ones(B, H_kv, device=DEV), vd)),
             ((vd[0], kd[1]), (full(vd[0]), full(kd[1])))]         # (H_kv,) broadcasts over B; different tensors
    for n in (1, 3):
        call = lambda k, v: fa.flash_attention_kvcache_forward(Q, K8, V8, lens, DEV, causal=True, scale=0.11, num_splits=n,
                                                               variant=variant, k_descale=k, v_descale=v)
        results = []
        for short, explicit in pairs:
            (O, L), (Oe, Le) = call(*short), call(*explicit)
            assert same_bits(O, Oe) and same_bits(L, Le), (fmt, variant, n, [None if t is None else tuple(t.shape) for t in short])
            results.append(O)
        assert not torch.equal(results[5], results[6])             # ... and do reach the result
        check_forward(*call(kd, vd), *truth(Q, K8, V8, kd, vd, [600, 129, 5], True, 0.11, None), BF16, (fmt, variant, n))


# (dtype, variant, d, g, N_q): the matrix form at d 64 and 128 with one and with two 32-row blocks, and the VALU form
IDENTITY = [(BF16, "mfma16", 128, 4, 1), (F16, "mfma16", 128, 8, 5), (F16, "mfma16", 64, 4, 2), (BF16, "mfma16", 64, 32, 2),
            (BF16, "generic", 64, 4, 2), (F16, "generic", 40, 2, 3)]


@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("dtype,variant,d,g,N_q", IDENTITY)
def test_identity_with_the_16_bit_path(dtype, variant, d, g, N_q, fmt):
    """Both descales None: O and L are, bit for bit, the 16-bit call's on the converted cache -- only staging changed."""
    lens, H_kv, S_k = [0, 1, 63, 64, 65, 1000, 777], 2, 1000
    Q, K8, V8, _, _ = quantized(len(lens), g * H_kv, H_kv, N_q, S_k, d, dtype, fmt, 3 * d + g)
    K16, V16 = K8.to(dtype), V8.to(dtype)
    assert torch.equal(K16.float(), K8.float())
    scale = 0.002 if fmt == E4 else 2e-5  # the raw cache values reach 448 / 57344
    for n in (1, 3, 16):
        for causal, window in ((True, None), (False, (100, 50))):
            O, L = fa.flash_attention_kvcache_forward(Q, K8, V8, lens_of(lens), DEV, causal=causal, scale=scale, window=window,
                                                      num_splits=n, variant=variant)
            O16, L16 = fa.flash_attention_kvcache_forward(Q, K16, V16, lens_of(lens), DEV, causal=causal, scale=scale, window=window,
                                                          num_splits=n, variant=variant)
            assert same_bits(O, O16) and same_bits(L, L16), (dtype, variant, d, g, N_q, fmt, n, causal, window)
    # exact fp32 descales: the truth bars (identity is not required here)
    Qs, K8s, V8s, kd, vd = quantized(len(lens), g * H_kv, H_kv, N_q, S_k, d, dtype, fmt, 3 * d + g + 1)
    K8s, V8s = (K8s.float() * kd[:, :, None, None] * 4).to(fmt), (V8s.float() * vd[:, :, None, None] / 4).to(fmt)
    kq, vq = torch.tensor(0.25, device=DEV), torch.tensor(4.0, device=DEV)
    for n in (1, 3):
        O, L = fa.flash_attention_kvcache_forward(Qs, K8s, V8s, lens_of(lens), DEV, causal=True, scale=d ** -0.5, num_splits=n,
                                                  variant=variant, k_descale=kq, v_descale=vq)
        check_forward(O, L, *truth(Qs, K8s, V8s, kq, vq, lens, True, d ** -0.5, None), dtype, ("0.25 / 4", dtype, variant, d, fmt, n))


@pytest.mark.parametrize("variant,d", [("mfma16", 128), ("mfma16", 64), ("generic", 64)])
@pytest.mark.parametrize("fmt", [E4, E5])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_every_finite_byte_is_staged_exactly(dtype, fmt, variant, d):
    """A cache that holds each finite byte pattern of the format, subnormals included, at every position of a 16-element load:
    bit-identical to the 16-bit call on the converted cache."""
    B, H, H_kv, N_q, S_k = 2, 8, 2, 1, 320
    b = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    b = b[torch.isfinite(b.view(fmt).float())]
    g = torch.Generator().manual_seed(d)
    idx = torch.randint(0, b.numel(), (2, B, H_kv, S_k, d), generator=g)
    idx[0].view(-1)[:17 * b.numel()] = torch.arange(b.numel()).repeat_interleave(17)  # every byte at every offset modulo 16
    idx[1].view(-1)[:17 * b.numel()] = torch.arange(b.numel()).repeat_interleave(17)
    K8, V8 = b[idx[0]].to(DEV).view(fmt), b[idx[1]].to(DEV).view(fmt)
    Q = (torch.randn(B, H, N_q, d, generator=g) * 0.5).to(dtype).to(DEV)
    scale = 1e-3 if fmt == E4 else 1e-5
    for n in (1, 2):
        O, L = fa.flash_attention_kvcache_forward(Q, K8, V8, None, DEV, scale=scale, num_splits=n, variant=variant)
        O16, L16 = fa.flash_attention_kvcache_forward(Q, K8.to(dtype), V8.to(dtype), None, DEV, scale=scale, num_splits=n,
                                                      variant=variant)
        assert not torch.isnan(O.float()).any() and same_bits(O, O16) and same_bits(L, L16), (dtype, fmt, variant, d, n)


@pytest.mark.parametrize("variant", ["mfma16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5])
def test_stale_rows_with_nan_and_inf_bytes_do_not_reach_the_output(fmt, variant):
    lens, H, H_kv, d = [0, 1, 63, 64, 65, 1000, 300, 511], 8, 2, 128
    for N_q, causal, window, n in ((1, False, None, 1), (3, True, None, 1), (2, False, (100, 50), 4), (1, False, None, 128)):
        Q, K8, V8, kd, vd = quantized(len(lens), H, H_kv, N_q, 1024, d, BF16, fmt, 5)
        outs = []
        for byte in (0,) + POISON:
            Kf, Vf = K8.clone().view(torch.uint8), V8.clone().view(torch.uint8)
            for b, nk in enumerate(lens):
                Kf[b, :, nk:] = byte
                Vf[b, :, nk:] = byte
            outs.append(fa.flash_attention_kvcache_forward(Q, Kf.view(fmt), Vf.view(fmt), lens_of(lens), DEV, causal=causal,
                                                           window=window, scale=0.1, num_splits=n, variant=variant, k_descale=kd,
                                                           v_descale=vd))
        for O, L in outs[1:]:
            assert not torch.isnan(O).any() and not torch.isnan(L).any()
            assert same_bits(O, outs[0][0]) and same_bits(L, outs[0][1]), (fmt, variant, N_q, causal, window, n)


@pytest.mark.parametrize("variant", ["auto", "generic", "mfma16"])
@pytest.mark.parametrize("num_splits", [0, 1, 5])
def test_empty_rows_are_exact(variant, num_splits):
    lens, N_q, H, H_kv, d = [0, 3, 10, 0], 5, 8, 2, 64
    Q, K8, V8, kd, vd = quantized(4, H, H_kv, N_q, 256, d, BF16, E4, 3)
    O, L = fa.flash_attention_kvcache_forward(Q, K8, V8, lens_of(lens), DEV, causal=True, num_splits=num_splits, variant=variant,
                                              k_descale=kd, v_descale=vd)
    for b, rows in ((0, range(5)), (1, range(2)), (3, range(5))):
        for q in rows:
            assert (O[b, :, q] == 0).all() and torch.isinf(L[b, :, q]).all() and (L[b, :, q] > 0).all(), (b, q)
    assert torch.isfinite(L[1, :, 2:]).all() and torch.isfinite(L[2]).all()
    check_forward(O, L, *truth(Q, K8, V8, kd, vd, lens, True, 1.0, None), BF16, (variant, num_splits))


@pytest.mark.parametrize("fmt,variant", [(E4, "mfma16"), (E5, "mfma16"), (E4, "generic")])
def test_workspace_poison_determinism_and_canaries(fmt, variant):
    B, H, H_kv, N_q, S_k, d = 5, 8, 2, 3, 700, 64
    lens = lens_of([0, 17, 700, 333, 64])
    Q, K8, V8, kd, vd = quantized(B, H, H_kv, N_q, S_k, d, BF16, fmt, 9)
    enum, kv_enum = convert_triton_dtype(BF16), convert_triton_dtype(fmt)
    for n in (4, 128):
        words = _lib.kvcache_workspace_bytes(B, H, N_q, d, n) // 4
        results = []
        for poison in (0.0, float("nan"), float("nan")):
            O, O_all, O_sl = arena(B * H * N_q * d, BF16, 77.0)
            L, L_all, L_sl = arena(B * H * N_q, BF16, 77.0)
            ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
            ws.fill_(poison)
            O4, L3 = O.view(B, H, N_q, d), L.view(B, H, N_q)
            _lib.fa2_fwd_kvcache_fp8(Q, K8, V8, O4, L3, lens, enum, kv_enum, k_descale=kd, v_descale=vd, causal=True, scale=0.1,
                                     num_splits=n, workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
            assert not torch.isnan(ws).any()  # every (split, row) partial was written
            results.append((O4.clone(), L3.clone()))
        for O4, L3 in results[1:]:  # NaN-poisoned == zeroed workspace, and the same call twice
            assert same_bits(O4, results[0][0]) and same_bits(L3, results[0][1]), (fmt, variant, n)
    # num_splits = 1: a poisoned workspace is neither read nor written
    O_ref, L_ref = fa.flash_attention_kvcache_forward(Q, K8, V8, lens, DEV, causal=True, scale=0.1, num_splits=1, variant=variant,
                                                      k_descale=kd, v_descale=vd)
    ws, ws_all, ws_sl = arena(1000, torch.float32, 77.0)
    ws.fill_(float("nan"))
    O4, L3 = torch.empty_like(O_ref), torch.empty_like(L_ref)
    _lib.fa2_fwd_kvcache_fp8(Q, K8, V8, O4, L3, lens, enum, kv_enum, k_descale=kd, v_descale=vd, causal=True, scale=0.1, num_splits=1,
                             workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and canaries_intact(ws_all, ws_sl, 77.0)
    assert same_bits(O4, O_ref) and same_bits(L3, L_ref)


@pytest.mark.parametrize("fmt,variant", [(E4, "auto"), (E5, "auto"), (E4, "generic")])
def test_bshd_cache_layout(fmt, variant):
    B, H, H_kv, N_q, S_k, d = 3, 8, 2, 2, 600, 128
    Q, K8, V8, kd, vd = quantized(B, H, H_kv, N_q, S_k, d, F16, fmt, 21)
    lens = [600, 129, 5]
    bshd = lambda t: t.view(torch.uint8).transpose(1, 2).contiguous().view(fmt)  # (B, S, H_kv, d) storage
    Kc, Vc = bshd(K8), bshd(V8)
    assert Kc.shape == (B, S_k, H_kv, d)
    for ln in (lens, None):
        O, L = fa.flash_attention_kvcache_forward(Q, Kc.transpose(1, 2), Vc.transpose(1, 2), None if ln is None else lens_of(ln),
                                                  DEV, causal=True, scale=0.09, num_splits=3, variant=variant, k_descale=kd,
                                                  v_descale=vd)
        check_forward(O, L, *truth(Q, K8, V8, kd, vd, ln, True, 0.09, None), F16, (fmt, variant, ln))


def test_forced_mfma16_rejections_and_auto_runs_them():
    for d, H, H_kv, N_q, pad in ((40, 8, 2, 1, 0), (64, 40, 1, 2, 0), (64, 8, 2, 1, 8)):
        Q, K8, V8, kd, vd = quantized(2, H, H_kv, N_q, 300, d, BF16, E4, 41)
        if pad:  # misaligned rows
            K8, V8 = strided_copy(K8, "row_stride"), strided_copy(V8, "row_stride")
        lens = lens_of([300, 77])
        with pytest.raises(TypeError, match="mfma16"):  # FA2_ERR_UNSUPPORTED
            fa.flash_attention_kvcache_forward(Q, K8, V8, lens, DEV, variant="mfma16", k_descale=kd, v_descale=vd)
        O, L = fa.flash_attention_kvcache_forward(Q, K8, V8, lens, DEV, scale=0.1, num_splits=2, k_descale=kd, v_descale=vd)
        check_forward(O, L, *truth(Q, K8, V8, kd, vd, [300, 77], False, 0.1, None), BF16, ("auto", d, H, H_kv, N_q, pad))
