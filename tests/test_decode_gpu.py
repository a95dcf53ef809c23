"""KV-cache decode attention (fa2_fwd_kvcache) on the GPU: O and L against the fp64 per-sequence truth over the first N_k(b) keys
for every variant, dtype, group size, N_q, mask and split count; exact empty rows; stale cache rows and a poisoned workspace
that must not reach the output; canary arenas; cache and query layouts; parity with the packed varlen call; forced-variant
rejections; one cache whose extent exceeds 32-bit byte offsets."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_bwd_arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the bars of tests/test_varlen_gpu.py: O_TOL, and for L 5e-5 relative (f32 / f64) or 1.01 ulp (16-bit)
O_TOL = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 5e-2, torch.float64: 1e-6}
S_K = 4200
LENS = [0, 1, 63, 64, 65, 1000, 4097, S_K]
WINDOWS = (None, (64, 0), (100, 50))
SPLITS = (0, 1, 2, 3, 7, 16, 128)


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def ulp(dtype, x):
    mant = {torch.float16: 10, torch.bfloat16: 7}[dtype]
    return 2.0 ** (math.floor(math.log2(max(abs(x), 1e-30))) - mant)


def make(B, H, H_kv, N_q, S_k, d, dtype, seed, amp=0.5):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randn(B, H, N_q, d, generator=g) * amp).to(dtype).to(DEV)
    K = (torch.randn(B, H_kv, S_k, d, generator=g) * amp).to(dtype).to(DEV)
    V = (torch.randn(B, H_kv, S_k, d, generator=g) * amp).to(dtype).to(DEV)
    return Q, K, V


def reference(Q, K, V, lens, causal, scale, window, heads=None):
    """fp64 truth, one sequence at a time, over the first N_k(b) keys: O (B, H, N_q, d), L (B, H, N_q); rows without a visible
    key get O = 0 and L = +inf.  heads: only these query heads (the large-offset case)."""
    B, H, N_q, d = Q.shape
    H_kv, S_k = K.shape[1], K.shape[2]
    g = H // H_kv
    hs = list(range(H)) if heads is None else list(heads)
    O = torch.zeros(B, len(hs), N_q, d, dtype=torch.float64, device=DEV)
    L = torch.full((B, len(hs), N_q), math.inf, dtype=torch.float64, device=DEV)
    for b in range(B):
        nk = S_k if lens is None else min(max(int(lens[b]), 0), S_k)
        m = fa2_bwd_arith.band(N_q, nk, causal, window, DEV)
        vis = m.any(-1)
        for n, h in enumerate(hs):
            q, k, v = Q[b, h].double(), K[b, h // g, :nk].double(), V[b, h // g, :nk].double()
            S = (q @ k.T) * f32(scale)
            S = S.masked_fill(~m, float("-inf"))
            P = torch.where(vis.view(N_q, 1), torch.softmax(S.masked_fill(~vis.view(N_q, 1), 0.0), -1), 0.0)
            O[b, n] = P @ v
            L[b, n] = torch.where(vis, torch.logsumexp(S, -1) * math.log2(math.e), math.inf)
    return O, L


def check_forward(O, L, O_ref, L_ref, dtype, what):
    O, L = O.double(), L.double()
    assert not torch.isnan(O).any() and not torch.isnan(L).any(), what
    empty = torch.isinf(L_ref)
    assert torch.equal(torch.isinf(L), empty) and (L[empty] > 0).all(), what  # exactly the empty rows, +inf
    assert (O[empty] == 0).all(), what
    err = (O - O_ref).abs().max().item()
    print(f"{what}: max|O - truth| = {err:.3e} (bar {O_TOL[dtype]:.0e})")
    assert err <= O_TOL[dtype], what
    Lf, Lr = L[~empty], L_ref[~empty]
    if Lr.numel() == 0:
        return
    if dtype in (torch.float32, torch.float64):
        assert ((Lf - Lr).abs() <= 5e-5 * Lr.abs().clamp(min=1)).all(), what
    else:
        assert (Lf - Lr).abs().max() <= 1.01 * ulp(dtype, Lr.abs().max().item()), what


def lens_of(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# (g, N_q, causal, window, num_splits): every g, N_q, window and split count of the issue, causal on and off, g * N_q <= 64
CONFIGS = [(4, 1, False, None, 0), (1, 2, True, None, 1), (8, 5, False, (64, 0), 2), (32, 1, False, (100, 50), 3),
           (4, 16, True, (64, 0), 7), (8, 1, False, None, 16), (1, 16, True, (100, 50), 128), (4, 5, True, None, 3),
           (32, 2, False, None, 128), (8, 2, True, (100, 50), 0), (1, 1, False, (64, 0), 16), (4, 2, False, (100, 50), 1)]
CASES = [(dt, v, d) for dt in (torch.float16, torch.bfloat16) for v in ("auto", "generic", "mfma16") for d in (64, 128)]
CASES += [(dt, v, d) for dt in (torch.float32, torch.float64) for v in ("auto", "generic") for d in (64, 40)]


@pytest.mark.parametrize("dtype,variant,d", CASES)
def test_forward_against_fp64_truth(dtype, variant, d):
    H_kv = 2
    scale = 1.0 / math.sqrt(d)
    lens = lens_of(LENS)
    assert {c[0] for c in CONFIGS} == {1, 4, 8, 32} and {c[1] for c in CONFIGS} == {1, 2, 5, 16}
    assert {c[3] for c in CONFIGS} == set(WINDOWS) and {c[4] for c in CONFIGS} == set(SPLITS)
    for g, N_q, causal, window, n in CONFIGS:
        Q, K, V = make(len(LENS), g * H_kv, H_kv, N_q, S_K, d, dtype, 7 * d + g + N_q)
        O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, causal=causal, scale=scale, window=window, num_splits=n,
                                                  variant=variant)
        assert O.shape == Q.shape and L.shape == Q.shape[:3] and O.dtype == dtype and L.dtype == dtype
        O_ref, L_ref = reference(Q, K, V, LENS, causal, scale, window)
        check_forward(O, L, O_ref, L_ref, dtype, (dtype, variant, d, g, N_q, causal, window, n))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("d", [256, 512])
def test_large_head_sizes_on_the_valu_form(dtype, d):
    """d > 128: four and eight output columns per lane; f64 at d = 512 asks for more than 64 KiB of LDS."""
    lens, H, H_kv, N_q = [0, 65, 300, 1000], 4, 2, 3
    Q, K, V = make(len(lens), H, H_kv, N_q, 1000, d, dtype, d)
    for n, causal, window in ((1, True, None), (3, False, (100, 50)), (0, False, None)):
        O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, causal=causal, scale=d ** -0.5, window=window,
                                                  num_splits=n)
        check_forward(O, L, *reference(Q, K, V, lens, causal, d ** -0.5, window), dtype, (dtype, d, n, causal, window))


@pytest.mark.parametrize("variant", ["auto", "generic", "mfma16"])
@pytest.mark.parametrize("num_splits", [0, 1, 5])
def test_empty_rows_are_exact(variant, num_splits):
    lens, N_q, H, H_kv, d = [0, 3, 10, 0], 5, 8, 2, 64
    Q, K, V = make(4, H, H_kv, N_q, 256, d, torch.bfloat16, 3)
    O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, causal=True, num_splits=num_splits, variant=variant)
    # cache_seqlens = 0: every row empty; causal with N_q = 5 > N_k = 3: rows 0 and 1 see no key
    for b, rows in ((0, range(5)), (1, range(2)), (3, range(5))):
        for q in rows:
            assert (O[b, :, q] == 0).all() and torch.isinf(L[b, :, q]).all() and (L[b, :, q] > 0).all(), (b, q)
    assert torch.isfinite(L[1, :, 2:]).all() and torch.isfinite(L[2]).all()
    check_forward(O, L, *reference(Q, K, V, lens, True, 1.0, None), torch.bfloat16, (variant, num_splits))


@pytest.mark.parametrize("dtype,variant", [(torch.bfloat16, "mfma16"), (torch.float16, "auto"), (torch.bfloat16, "generic"),
                                           (torch.float32, "auto")])
def test_stale_cache_rows_do_not_reach_the_output(dtype, variant):
    lens, H, H_kv, d = [0, 1, 63, 64, 65, 1000, 300, 511], 8, 2, 128
    for N_q, causal, window, n in ((1, False, None, 0), (3, True, None, 1), (2, False, (100, 50), 4), (1, False, None, 128)):
        Q, K, V = make(len(lens), H, H_kv, N_q, 1024, d, dtype, 5)
        outs = []
        for fill in (0.0, float("nan"), float("inf"), float("-inf")):
            Kf, Vf = K.clone(), V.clone()
            for b, nk in enumerate(lens):
                Kf[b, :, nk:] = fill
                Vf[b, :, nk:] = fill
            outs.append(fa.flash_attention_kvcache_forward(Q, Kf, Vf, lens_of(lens), DEV, causal=causal, window=window, scale=0.1,
                                                           num_splits=n, variant=variant))
        for O, L in outs[1:]:
            assert not torch.isnan(O).any() and not torch.isnan(L).any()
            assert torch.equal(O, outs[0][0]) and torch.equal(L, outs[0][1]), (N_q, causal, window, n)


def arena(numel, dtype, value):
    """A tensor of `numel` elements inside a canary arena: (view, whole arena, slice of the view)."""
    pad = 4096
    whole = torch.full((numel + 2 * pad,), value, dtype=dtype, device=DEV)
    return whole[pad:pad + numel], whole, slice(pad, pad + numel)


def canaries_intact(whole, sl, value):
    outside = torch.cat([whole[:sl.start], whole[sl.stop:]])
    return bool((outside == value).all())


@pytest.mark.parametrize("dtype,variant", [(torch.bfloat16, "mfma16"), (torch.bfloat16, "generic"), (torch.float32, "generic")])
def test_workspace_poison_determinism_and_canaries(dtype, variant):
    B, H, H_kv, N_q, S_k, d = 5, 8, 2, 3, 700, 64
    lens = lens_of([0, 17, 700, 333, 64])
    Q, K, V = make(B, H, H_kv, N_q, S_k, d, dtype, 9)
    enum = convert_triton_dtype(dtype)
    for n in (4, 128):
        words = _lib.kvcache_workspace_bytes(B, H, N_q, d, n) // 4
        results = []
        for poison in (0.0, float("nan"), float("nan")):
            O, O_all, O_sl = arena(B * H * N_q * d, dtype, 77.0)
            L, L_all, L_sl = arena(B * H * N_q, dtype, 77.0)
            ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
            ws.fill_(poison)
            O4, L3 = O.view(B, H, N_q, d), L.view(B, H, N_q)
            _lib.fa2_fwd_kvcache(Q, K, V, O4, L3, lens, enum, causal=True, scale=0.1, num_splits=n, workspace=ws,
                                 variant=_lib.KVCACHE_VARIANTS[variant])
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
            assert not torch.isnan(ws).any()  # every (split, row) partial was written
            results.append((O4.clone(), L3.clone()))
        for O4, L3 in results[1:]:  # NaN-poisoned == zeroed workspace, and the same call twice
            assert torch.equal(O4, results[0][0]) and torch.equal(L3, results[0][1]), (variant, n)
    # num_splits = 1: a poisoned workspace of any size is neither read nor written
    O_ref, L_ref = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, causal=True, scale=0.1, num_splits=1, variant=variant)
    for words in (1, 1000, _lib.kvcache_workspace_bytes(B, H, N_q, d, 8) // 4):
        ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
        ws.fill_(float("nan"))
        O4, L3 = torch.empty_like(O_ref), torch.empty_like(L_ref)
        _lib.fa2_fwd_kvcache(Q, K, V, O4, L3, lens, enum, causal=True, scale=0.1, num_splits=1, workspace=ws,
                             variant=_lib.KVCACHE_VARIANTS[variant])
        torch.cuda.synchronize()
        assert torch.isnan(ws).all() and canaries_intact(ws_all, ws_sl, 77.0)
        assert torch.equal(O4, O_ref) and torch.equal(L3, L_ref)


@pytest.mark.parametrize("dtype,variant", [(torch.bfloat16, "auto"), (torch.bfloat16, "generic"), (torch.float32, "auto")])
def test_cache_and_query_layouts(dtype, variant):
    B, H, H_kv, N_q, S_k, d = 3, 8, 2, 2, 600, 128
    Q, K, V = make(B, H, H_kv, N_q, S_k, d, dtype, 21)
    lens = [600, 129, 5]
    bshd = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)  # (B, S, H, d) storage, (B, H, S, d) view
    for qf in (lambda t: t, bshd):
        for kf in (lambda t: t, bshd):
            for ln in (lens, None):
                Qx, Kx, Vx = qf(Q), kf(K), kf(V)
                O, L = fa.flash_attention_kvcache_forward(Qx, Kx, Vx, None if ln is None else lens_of(ln), DEV, causal=True,
                                                          scale=0.09, num_splits=3, variant=variant)
                check_forward(O, L, *reference(Q, K, V, ln, True, 0.09, None), dtype, (variant, Qx.stride(), Kx.stride(), ln))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_parity_with_the_packed_varlen_call(dtype):
    B, H, H_kv, N_q, N_k, d = 3, 8, 2, 4, 777, 64
    Q, K, V = make(B, H, H_kv, N_q, N_k, d, dtype, 33)
    pack = lambda t: t.transpose(1, 2).reshape(B * t.shape[2], t.shape[1], d).contiguous()
    cu = lambda n: torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=DEV)
    for causal, window in ((False, None), (True, None), (False, (64, 0))):
        Ov, Lv = fa.flash_attention_varlen_forward(pack(Q), pack(K), pack(V), cu(N_q), cu(N_k), N_q, N_k, DEV, causal=causal,
                                                   scale=0.1, window=window)
        for n in (1, 0, 5):
            O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens_of([N_k] * B), DEV, causal=causal, scale=0.1, window=window,
                                                      num_splits=n)
            O_ref = Ov.view(B, N_q, H, d).transpose(1, 2).double()
            L_ref = Lv.view(H, B, N_q).transpose(0, 1).double()
            check_forward(O, L, O_ref, L_ref, dtype, ("varlen parity", dtype, causal, window, n))


def test_forced_mfma16_rejections_and_auto_runs_them():
    for dtype, d, H, H_kv, N_q in ((torch.float32, 64, 8, 2, 1), (torch.bfloat16, 40, 8, 2, 1), (torch.bfloat16, 64, 40, 1, 2)):
        Q, K, V = make(2, H, H_kv, N_q, 300, d, dtype, 41)
        lens = lens_of([300, 77])
        with pytest.raises(TypeError):  # FA2_ERR_UNSUPPORTED
            fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, variant="mfma16")
        O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, scale=0.1, num_splits=2)
        check_forward(O, L, *reference(Q, K, V, [300, 77], False, 0.1, None), dtype, ("auto", dtype, d, H, H_kv, N_q))


def test_cache_extent_beyond_32_bit_byte_offsets():
    H, H_kv, d = 16, 8, 128
    S = (1 << 21) + 192  # S_k x row stride (8 * 128 elements of 2 bytes) > 2^32 bytes
    K = torch.empty(1, S, H_kv, d, dtype=torch.bfloat16, device=DEV).normal_(0, 0.5)
    V = torch.empty(1, S, H_kv, d, dtype=torch.bfloat16, device=DEV).normal_(0, 0.5)
    assert S * K.stride(1) * 2 > 1 << 32
    Q = (torch.randn(1, H, 1, d) * 0.5).to(torch.bfloat16).to(DEV)
    nk = S - 3
    O, L = fa.flash_attention_kvcache_forward(Q, K.transpose(1, 2), V.transpose(1, 2), lens_of([nk]), DEV, scale=0.09)
    heads = (14, 15)  # the last KV group: its keys end beyond the 4 GiB mark
    O_ref, L_ref = reference(Q, K.transpose(1, 2), V.transpose(1, 2), [nk], False, 0.09, None, heads=heads)
    check_forward(O[:, 14:], L[:, 14:], O_ref, L_ref, torch.bfloat16, "large offsets")


def test_split_versus_unsplit_difference_is_reported():
    """A measurement, not a bar: the largest difference between a split and the unsplit result, in ulps of the output dtype."""
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        Q, K, V = make(4, 32, 8, 1, 8192, 128, dtype, 51)
        lens = lens_of([8192, 5000, 100, 8191])
        O1, L1 = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, scale=0.09, num_splits=1)
        worst = 0.0
        for n in (2, 7, 16, 128):
            O, _ = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, scale=0.09, num_splits=n)
            u = fa2_bwd_arith.ulp(O1.double().abs().amax(-1, keepdim=True), dtype)  # one ulp at the row's largest |O|
            worst = max(worst, ((O.double() - O1.double()).abs() / u).max().item())
        print(f"split vs unsplit, {dtype}: largest difference {worst:.2f} ulps of the row's largest output")
        assert math.isfinite(worst)
