"""Paged KV-cache decode (fa2_fwd_kvcache_paged) on the GPU.  The yardstick is bit-equality with the contiguous call on the cache
the pool was scattered from; beside it the fp64 truth over the gathered keys, fills of everything that must not matter (unused
pages, rows behind N_k(b), table entries past a sequence's pages), shared pages, pool and table layouts, a pool beyond 32-bit byte
offsets, and canary arenas around O, L, the workspace and the pool.

The pool always holds more pages than are used and the table entries past a sequence's pages are -1 and 2^31 - 1: the kernels
clamp every entry they read into the pool, so no access outside it can occur."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_bwd_arith

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the bars of tests/test_decode_gpu.py: O_TOL, and for L 5e-5 relative (f32 / f64) or 1.01 ulp (16-bit)
O_TOL = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 5e-2, torch.float64: 1e-6}
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
INT_MAX = 2 ** 31 - 1
H_KV = 2
SPARE = 5  # pool pages no table names


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


def fill_value(dtype, fill):
    """`fill` in the pool's dtype; an fp8 pool is filled through its bytes (0x7F is NaN in both formats, 0x7C +inf in e5m2 and a
    large finite number in e4m3fn, which has no inf)."""
    if dtype in (E4, E5):
        return 0x7F if fill != fill else (0x7C if fill == math.inf else 0)
    return fill


def scatter(K, V, P, lens, seed, fill=float("nan"), tail=(-1, INT_MAX)):
    """A contiguous (B, H_kv, S_k, d) cache, S_k = max_blocks * P, scattered into pools of B * max_blocks + SPARE pages under a
    seeded random permutation table -> (K_pool, V_pool, table).  Unused pages and the rows at or past N_k(b) of a last page hold
    `fill`; table entries past a sequence's pages hold the values of `tail` in turn."""
    B, H_kv, S_k, d = K.shape
    mb = S_k // P
    assert mb * P == S_k
    nb = B * mb + SPARE
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    table = perm[:B * mb].view(B, mb).clone()
    pools = []
    for t in (K, V):
        raw = t.view(torch.uint8) if t.dtype in (E4, E5) else t
        fv = fill_value(t.dtype, fill)
        src = raw.clone()
        for b, n in enumerate(lens):
            src[b, :, n:] = fv
        pool = torch.full((nb, H_kv, P, d), fv, dtype=raw.dtype, device=DEV)
        pool[table.view(-1).long().to(DEV)] = src.view(B, H_kv, mb, P, d).permute(0, 2, 1, 3, 4).reshape(B * mb, H_kv, P, d)
        pools.append(pool.view(t.dtype))
    for b, n in enumerate(lens):
        used = -(-n // P)
        for i in range(used, mb):
            table[b, i] = tail[(i - used) % len(tail)]
    return pools[0], pools[1], table.to(DEV)


def gather(pool, table, nb):
    """The keys a table names, as a contiguous (B, H_kv, max_blocks * P, d) cache (entries clamped as the kernels clamp them)."""
    B, mb = table.shape
    _, H_kv, P, d = pool.shape
    raw = pool.view(torch.uint8) if pool.dtype in (E4, E5) else pool
    pages = raw[table.long().clamp(0, nb - 1).view(-1)].view(B, mb, H_kv, P, d)
    return pages.permute(0, 2, 1, 3, 4).reshape(B, H_kv, mb * P, d).view(pool.dtype)


def lengths(P, cap):
    return [min(n, cap) for n in (0, 1, P - 1, P, P + 1, 2 * P + 63, cap)]


def problem(dtype, kv, d, P, g, N_q, seed):
    """Q, the contiguous cache (quantised for an fp8 `kv`, with per-(b, h_kv) descales) and its lengths: B = 7, capacity about
    1024 keys, or 16 pages for the small page sizes."""
    cap = 16 * P if P < 64 else 1024
    lens = lengths(P, cap)
    Q, K, V = make(len(lens), g * H_KV, H_KV, N_q, cap, d, dtype, seed)
    kd = vd = None
    if kv is not None:
        K, kd = fa.quantize_kv_cache(K, kv)
        V, vd = fa.quantize_kv_cache(V, kv)
    return Q, K, V, kd, vd, lens


def both(Q, K, V, Kp, Vp, table, lens, **kw):
    """(paged result, contiguous result) of one call."""
    paged = fa.flash_attention_kvcache_forward(Q, Kp, Vp, lens, DEV, block_table=table, **kw)
    flat = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, **kw)
    return paged, flat


def assert_equal(paged, flat, what):
    assert not torch.isnan(paged[0]).any() and not torch.isnan(paged[1]).any(), what
    assert torch.equal(paged[0], flat[0]), what
    assert torch.equal(paged[1], flat[1]), what


# (variant, dtype, fp8 pool format, d, page_size, g, N_q, causal, window, num_splits).  g * N_q = 40 is beyond the issue's list:
# it is the smallest shape on the two-row-block instantiations of the matrix form.  The auto cases are ones where auto takes the
# same form on both sides (a 16-bit pool of sub-64 pages goes to the VALU form, its contiguous cache to the matrix form: that
# case is compared with the contiguous generic call in test_forced_mfma16_needs_pages_of_a_multiple_of_64_and_auto_runs_them).
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CONFIGS = [
    ("mfma16", BF, None, 128, 64, 4, 1, False, None, 1), ("mfma16", F16, None, 64, 128, 1, 5, True, None, 3),
    ("mfma16", BF, None, 64, 256, 32, 1, False, (100, 50), 16), ("mfma16", F16, None, 128, 256, 4, 5, True, (100, 50), 3),
    ("mfma16", BF, None, 128, 128, 32, 1, True, None, 16), ("mfma16", F16, None, 128, 64, 8, 5, False, None, 3),
    ("mfma16", BF, None, 64, 64, 8, 5, True, None, 16),
    ("mfma16", BF, E4, 128, 64, 4, 1, False, None, 3), ("mfma16", BF, E5, 64, 128, 1, 5, True, (100, 50), 1),
    ("mfma16", BF, E4, 128, 256, 8, 5, True, None, 16),
    ("generic", BF, None, 64, 1, 4, 1, False, None, 1), ("generic", F32, None, 40, 16, 1, 5, True, None, 3),
    ("generic", BF, None, 40, 48, 32, 5, False, (100, 50), 16), ("generic", F32, None, 64, 64, 4, 1, True, (100, 50), 3),
    ("generic", F32, None, 64, 48, 32, 1, False, None, 16), ("generic", F32, None, 40, 1, 4, 5, True, None, 3),
    ("generic", BF, E4, 64, 16, 4, 5, True, None, 3), ("generic", BF, E5, 40, 48, 1, 1, False, None, 1),
    ("auto", BF, None, 128, 128, 4, 1, False, None, 0), ("auto", F32, None, 64, 16, 4, 1, True, None, 0),
    ("auto", F32, None, 64, 64, 1, 5, False, (100, 50), 0), ("auto", BF, E4, 128, 64, 32, 1, False, None, 0),
]


def test_configs_cover_the_issue():
    m = [c for c in CONFIGS if c[0] == "mfma16"]
    g = [c for c in CONFIGS if c[0] == "generic"]
    assert {c[1] for c in m} == {BF, F16} and {c[3] for c in m} == {64, 128} and {c[4] for c in m} == {64, 128, 256}
    assert {c[1] for c in g} == {BF, F32} and {c[3] for c in g} == {64, 40} and {c[4] for c in g} == {1, 16, 48, 64}
    assert {c[2] for c in m} == {None, E4, E5} and {c[2] for c in g} == {None, E4, E5}
    for cs in (m, g):
        assert {c[5] for c in cs} >= {1, 4, 32} and {c[6] for c in cs} == {1, 5} and {c[9] for c in cs} == {1, 3, 16}
        assert {c[7] for c in cs} == {False, True} and {c[8] for c in cs} == {None, (100, 50)}
    assert all(c[5] * c[6] <= 64 for c in m) and any(c[5] * c[6] > 32 for c in m)
    assert any(c[0] == "auto" and c[9] == 0 for c in CONFIGS)


@pytest.mark.parametrize("variant,dtype,kv,d,P,g,N_q,causal,window,n", CONFIGS)
def test_bit_equal_to_the_contiguous_call(variant, dtype, kv, d, P, g, N_q, causal, window, n):
    Q, K, V, kd, vd, lens = problem(dtype, kv, d, P, g, N_q, 7 * d + g + N_q + P)
    Kp, Vp, table = scatter(K, V, P, lens, seed=P + g)
    paged, flat = both(Q, K, V, Kp, Vp, table, lens_of(lens), causal=causal, window=window, scale=1.0 / math.sqrt(d), num_splits=n,
                       variant=variant, k_descale=kd, v_descale=vd)
    assert paged[0].shape == Q.shape and paged[1].shape == Q.shape[:3] and paged[0].dtype == dtype and paged[1].dtype == dtype
    assert_equal(paged, flat, (variant, dtype, kv, d, P, g, N_q, causal, window, n))


def test_all_keys_without_cache_seqlens():
    """cache_seqlens = None: every sequence uses the whole capacity max_blocks * page_size."""
    for variant, P in (("mfma16", 64), ("generic", 16)):
        Q, K, V = make(3, 8, H_KV, 1, 8 * P, 64, BF, 11)
        Kp, Vp, table = scatter(K, V, P, [8 * P] * 3, seed=1)
        paged, flat = both(Q, K, V, Kp, Vp, table, None, scale=0.1, num_splits=2, variant=variant)
        assert_equal(paged, flat, (variant, P))


@pytest.mark.parametrize("dtype,kv", [(BF, None), (F16, None), (F32, None), (BF, E4), (BF, E5)])
def test_against_fp64_truth_over_the_gathered_keys(dtype, kv):
    cases = [("generic", 40, 16, 4, 5, True, None, 3), ("generic", 64, 48, 1, 1, False, (100, 50), 1)]
    if dtype != F32:
        cases += [("mfma16", 128, 64, 4, 1, False, None, 3), ("mfma16", 64, 128, 8, 5, True, (100, 50), 16)]
    for variant, d, P, g, N_q, causal, window, n in cases:
        Q, K, V, kd, vd, lens = problem(dtype, kv, d, P, g, N_q, d + P)
        Kp, Vp, table = scatter(K, V, P, lens, seed=3 * P)
        O, L = fa.flash_attention_kvcache_forward(Q, Kp, Vp, lens_of(lens), DEV, causal=causal, window=window, scale=d ** -0.5,
                                                  num_splits=n, variant=variant, k_descale=kd, v_descale=vd, block_table=table)
        Kg, Vg = gather(Kp, table, Kp.shape[0]), gather(Vp, table, Vp.shape[0])
        if kv is not None:
            Kg, Vg = fa.dequantize_kv_cache(Kg, kd, torch.float64), fa.dequantize_kv_cache(Vg, vd, torch.float64)
        check_forward(O, L, *reference(Q, Kg, Vg, lens, causal, d ** -0.5, window), dtype, (dtype, kv, variant, d, P, g, N_q, n))


@pytest.mark.parametrize("variant,dtype,kv,P", [("mfma16", BF, None, 64), ("generic", BF, None, 48), ("generic", F32, None, 1),
                                                ("mfma16", F16, E5, 128), ("generic", BF, E4, 16)])
def test_what_must_not_matter(variant, dtype, kv, P):
    """Unused pages, the rows behind N_k(b) and the table entries past a sequence's pages: three fills, one result."""
    for N_q, causal, window, n in ((1, False, None, 3), (5, True, (100, 50), 1)):
        Q, K, V, kd, vd, lens = problem(dtype, kv, 64, P, 4, N_q, 5 + P)
        outs = []
        for fill, tail in ((0.0, (0,)), (float("nan"), (-1,)), (float("inf"), (INT_MAX,))):
            Kp, Vp, table = scatter(K, V, P, lens, seed=P, fill=fill, tail=tail)
            outs.append(fa.flash_attention_kvcache_forward(Q, Kp, Vp, lens_of(lens), DEV, causal=causal, window=window, scale=0.1,
                                                           num_splits=n, variant=variant, k_descale=kd, v_descale=vd,
                                                           block_table=table))
        for O, L in outs:
            assert not torch.isnan(O).any() and not torch.isnan(L).any()
        for O, L in outs[1:]:
            assert torch.equal(O, outs[0][0]) and torch.equal(L, outs[0][1]), (variant, P, N_q, n)


@pytest.mark.parametrize("variant,P", [("mfma16", 64), ("generic", 16), ("auto", 128)])
def test_shared_pages(variant, P):
    """Two sequences whose tables name the same pages for a common prefix of two pages, with different tails and lengths."""
    mb, d = 6, 64
    lens = [3 * P + 5, 5 * P - 1]
    Q, K, V = make(2, 8, H_KV, 1, mb * P, d, BF, 17)
    K[1, :, :2 * P] = K[0, :, :2 * P]
    V[1, :, :2 * P] = V[0, :, :2 * P]
    Kp, Vp, table = scatter(K, V, P, lens, seed=9)
    for pool in (Kp, Vp):  # sequence 1 reads its prefix through sequence 0's pages; its own copies become unused pages
        pool[table[1, :2].long()] = float("nan")
    table[1, :2] = table[0, :2]
    for causal, n in ((False, 1), (True, 3)):
        paged, flat = both(Q, K, V, Kp, Vp, table, lens_of(lens), causal=causal, scale=0.1, num_splits=n, variant=variant)
        assert_equal(paged, flat, (variant, P, causal, n))


@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_pool_and_table_layouts(variant):
    """A flash-attn (num_blocks, page_size, H_kv, d) pool as its transposed view, and a table that is a column slice of a wider
    tensor (row stride > max_blocks)."""
    P, d = 64, 128
    Q, K, V, _, _, lens = problem(BF, None, d, P, 4, 1, 23)
    Kp, Vp, table = scatter(K, V, P, lens, seed=4)
    nhd = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)  # (num_blocks, P, H_kv, d) storage
    wide = torch.full((table.shape[0], table.shape[1] + 7), -1, dtype=torch.int32, device=DEV)
    wide[:, 3:3 + table.shape[1]] = table
    sliced = wide[:, 3:3 + table.shape[1]]
    assert sliced.stride(0) > table.shape[1] and nhd(Kp).stride(2) == H_KV * d
    flat = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, scale=0.09, num_splits=3, variant=variant)
    for Kx, Vx, tx in ((nhd(Kp), nhd(Vp), table), (Kp, Vp, sliced), (nhd(Kp), Vp, sliced)):
        paged = fa.flash_attention_kvcache_forward(Q, Kx, Vx, lens_of(lens), DEV, scale=0.09, num_splits=3, variant=variant,
                                                   block_table=tx)
        assert_equal(paged, flat, (variant, Kx.stride(), tx.stride()))


def test_forced_mfma16_needs_pages_of_a_multiple_of_64_and_auto_runs_them():
    Q, K, V, _, _, lens = problem(BF, None, 64, 48, 4, 1, 29)
    Kp, Vp, table = scatter(K, V, 48, lens, seed=2)
    with pytest.raises(TypeError, match="page_size % 64"):  # FA2_ERR_UNSUPPORTED
        fa.flash_attention_kvcache_forward(Q, Kp, Vp, lens_of(lens), DEV, variant="mfma16", block_table=table)
    # auto takes the VALU form there, while the contiguous auto call takes the matrix form: equal to the contiguous generic call
    for n in (2, 0):
        paged = fa.flash_attention_kvcache_forward(Q, Kp, Vp, lens_of(lens), DEV, scale=0.1, num_splits=n, block_table=table)
        flat = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, scale=0.1, num_splits=n, variant="generic")
        assert_equal(paged, flat, ("auto at page_size 48", n))


def test_pool_beyond_32_bit_byte_offsets():
    H, H_kv, d, P = 16, 8, 128, 256
    nb = 8200
    Kp = torch.empty(nb, H_kv, P, d, dtype=BF, device=DEV)
    Vp = torch.empty(nb, H_kv, P, d, dtype=BF, device=DEV)
    assert nb * Kp.stride(0) * 2 > 1 << 32
    pages = [nb - 1, 5, nb - 2, 4100, nb - 3]  # only these are filled with data; the last ones end beyond the 4 GiB mark
    for pool in (Kp, Vp):
        pool[pages] = torch.empty(len(pages), H_kv, P, d, dtype=BF, device=DEV).normal_(0, 0.5)
    table = torch.tensor([pages + [-1, INT_MAX]], dtype=torch.int32, device=DEV)
    Q = (torch.randn(1, H, 1, d) * 0.5).to(BF).to(DEV)
    nk = len(pages) * P - 3
    O, L = fa.flash_attention_kvcache_forward(Q, Kp, Vp, lens_of([nk]), DEV, scale=0.09, block_table=table)
    idx = torch.tensor(pages, device=DEV)
    Kg = Kp[idx, H_kv - 1:].permute(1, 0, 2, 3).reshape(1, 1, len(pages) * P, d)  # the last KV head's keys, gathered
    Vg = Vp[idx, H_kv - 1:].permute(1, 0, 2, 3).reshape(1, 1, len(pages) * P, d)
    O_ref, L_ref = reference(Q[:, 14:], Kg, Vg, [nk], False, 0.09, None)  # the last KV group: heads 14 and 15
    check_forward(O[:, 14:], L[:, 14:], O_ref, L_ref, BF, "large offsets")


def arena(numel, dtype, value):
    """A tensor of `numel` elements inside a canary arena: (view, whole arena, slice of the view)."""
    pad = 4096
    whole = torch.full((numel + 2 * pad,), value, dtype=dtype, device=DEV)
    return whole[pad:pad + numel], whole, slice(pad, pad + numel)


def canaries_intact(whole, sl, value):
    outside = torch.cat([whole[:sl.start], whole[sl.stop:]])
    return bool((outside == value).all())


@pytest.mark.parametrize("variant,P", [("mfma16", 64), ("generic", 48)])
def test_workspace_poison_determinism_and_canaries(variant, P):
    B, H, N_q, d, dtype = 5, 8, 3, 64, BF
    lens = [0, 17, 12 * P, 333, 64]
    Q, K, V = make(B, H, H_KV, N_q, 12 * P, d, dtype, 9)
    Kp0, Vp0, table = scatter(K, V, P, lens, seed=6)
    # the pools inside arenas of their own: the kernels only read them, arena and pool must come back unchanged
    Kp, K_all, K_sl = arena(Kp0.numel(), dtype, 77.0)
    Vp, V_all, V_sl = arena(Vp0.numel(), dtype, 77.0)
    Kp.copy_(Kp0.view(-1))
    Vp.copy_(Vp0.view(-1))
    Kp, Vp = Kp.view(Kp0.shape), Vp.view(Vp0.shape)
    K_before, V_before = K_all.clone(), V_all.clone()
    enum = convert_triton_dtype(dtype)
    flat = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, causal=True, scale=0.1, num_splits=4, variant=variant)
    words = _lib.kvcache_workspace_bytes(B, H, N_q, d, 4) // 4
    results = []
    for poison in (0.0, float("nan"), float("nan")):
        O, O_all, O_sl = arena(B * H * N_q * d, dtype, 77.0)
        L, L_all, L_sl = arena(B * H * N_q, dtype, 77.0)
        ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
        ws.fill_(poison)
        O4, L3 = O.view(B, H, N_q, d), L.view(B, H, N_q)
        _lib.fa2_fwd_kvcache_paged(Q, Kp, Vp, O4, L3, table, lens_of(lens), enum, enum, causal=True, scale=0.1, num_splits=4,
                                   workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
        torch.cuda.synchronize()
        assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
        assert not torch.isnan(ws).any()  # every (split, row) partial was written
        results.append((O4.clone(), L3.clone()))
    for O4, L3 in results:  # NaN-poisoned == zeroed workspace, the same call twice, and the contiguous call
        assert torch.equal(O4, flat[0]) and torch.equal(L3, flat[1]), variant
    same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))  # bytes: the pool holds NaN
    assert same(K_all, K_before) and same(V_all, V_before)
