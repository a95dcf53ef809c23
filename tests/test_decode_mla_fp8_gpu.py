"""MLA decode over an fp8 latent cache (fa2_fwd_kvcache_mla_fp8) on the GPU with random data.  Truth is the fp64 reference of
tests/test_decode_mla_gpu.py on the DEQUANTISED cache descale * KV8.double(); the bars are tests/test_decode_gpu.py's own
(check_forward: O_TOL, L within 1.01 ulp): the kernels' arithmetic on the staged values is the 16-bit kernels' on an exactly
representable cache.  Also: bit-identity with the 16-bit path at descale None (only staging changed), every finite byte of each format
at every offset of a 16-element load and in the last 64 columns, stale rows filled with the formats' NaN / inf bytes, empty rows, a
poisoned workspace, determinism and canary arenas, paged against contiguous bit for bit, a V tensor of its own and (192, 128) on the
VALU form, two independent descales on one shared row, kv_descale broadcasting, and the 16-bit path through the new entry point."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_gpu import arena, canaries_intact, check_forward, lens_of
from test_decode_mla_gpu import make, reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
F16, BF16 = torch.float16, torch.bfloat16
S_K = 700
LENS = [0, 1, 63, 64, 65, 300, S_K]
SPLITS = (1, 3, 16)
SCALE = 576 ** -0.5
POISON = (0x7F, 0xFF, 0x7C, 0xFC)  # e4m3fn: NaN, NaN, 352, -352; e5m2: NaN, NaN, +inf, -inf
MLA = _lib.KVCACHE_MLA_VARIANTS

ids = lambda x: str(x).replace("torch.", "")


def quantized(B, H, N_q, S_k, dtype, fmt, seed, d=576, H_kv=1):
    """Q and an fp8 latent cache by the documented route: random rows, then quantize_kv_cache -> (B, H_kv) descales"""
    Q, KV = make(B, H, N_q, S_k, dtype, seed, d=d, H_kv=H_kv)
    KV8, kvd = fa.quantize_kv_cache(KV, fmt)
    return Q, KV8, kvd


def dequant(X8, descale):
    ones = torch.ones(X8.shape[:2], device=DEV)
    return X8.float().double() * (ones if descale is None else descale.expand_as(ones)).double()[:, :, None, None]


def truth(Q, KV8, kd, vd, lens, causal, scale, window, d_v=512, V8=None):
    """the fp64 reference on kd * K8 and vd * V8 (V8: the first d_v columns of the shared row unless given)"""
    return reference(Q, dequant(KV8, kd), dequant(KV8[..., :d_v] if V8 is None else V8, vd), lens, causal, scale, window)


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def launch(Q, K8, V8, lens, kd, vd, variant, n, causal=False, scale=SCALE, window=None, block_table=None, kv_enum=None):
    """fa2_fwd_kvcache_mla_fp8 itself (two descales, a V of its own): outputs and workspace allocated here -> (O, L)"""
    B, H, N_q, _ = Q.shape
    d_v = V8.shape[3]
    enum = convert_triton_dtype(Q.dtype)
    S = K8.shape[2] if block_table is None else block_table.shape[1] * K8.shape[2]
    n = n or _lib.kvcache_mla_num_splits(B, H, K8.shape[1], N_q, S, Q.shape[3], d_v, enum)
    O = torch.empty(B, H, N_q, d_v, dtype=Q.dtype, device=DEV)
    L = torch.empty(B, H, N_q, dtype=Q.dtype, device=DEV)
    ws = torch.empty(_lib.kvcache_workspace_bytes(B, H, N_q, d_v, n) // 4, dtype=torch.float32, device=DEV) if n > 1 else None
    view = lambda t: None if t is None else torch.broadcast_to(t, (B, K8.shape[1]))
    _lib.fa2_fwd_kvcache_mla_fp8(Q, K8, V8, O, L, lens, enum, convert_triton_dtype(K8.dtype) if kv_enum is None else kv_enum,
                                 k_descale=view(kd), v_descale=view(vd), block_table=block_table, causal=causal, scale=scale,
                                 window=window, num_splits=n, workspace=ws, variant=MLA[variant])
    return O, L


MASKS = ((False, None), (True, None), (False, (100, 50)))


@functools.lru_cache(maxsize=None)
def truth_case(H, N_q, dtype, fmt):
    """inputs and the fp64 truth under every mask of one shape: computed once, shared by the variants and split counts"""
    Q, KV8, kvd = quantized(len(LENS), H, N_q, S_K, dtype, fmt, 11 * H + N_q)
    return Q, KV8, kvd, {m: truth(Q, KV8, kvd, kvd, LENS, m[0], SCALE, m[1]) for m in MASKS}


@pytest.mark.parametrize("H,N_q", [(16, 1), (16, 2), (128, 1), (128, 2)])
@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_forward_against_fp64_truth(dtype, fmt, variant, H, N_q):
    lens = lens_of(LENS)
    Q, KV8, kvd, refs = truth_case(H, N_q, dtype, fmt)
    vals = kvd.flatten().tolist()
    assert kvd.shape == (len(LENS), 1) and len(set(vals)) > 1 and not any(math.log2(x).is_integer() for x in vals)
    for (causal, window), (O_ref, L_ref) in refs.items():
        for n in SPLITS:
            O, L = fa.flash_attention_mla_decode_forward(Q, KV8, lens, DEV, causal=causal, window=window, scale=SCALE, num_splits=n,
                                                         variant=variant, kv_descale=kvd)
            assert O.shape == (len(LENS), H, N_q, 512) and L.shape == (len(LENS), H, N_q) and O.dtype == dtype and L.dtype == dtype
            check_forward(O, L, O_ref, L_ref, dtype, (dtype, fmt, variant, H, N_q, causal, window, n))


@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
@pytest.mark.parametrize("dtype,H,N_q", [(BF16, 16, 1), (F16, 72, 2)], ids=ids)
def test_identity_with_the_16_bit_path(dtype, H, N_q, fmt, variant):
    """kv_descale None: O and L are, bit for bit, the 16-bit call's on the converted cache under the same variant and split count --
    only staging changed"""
    lens = [0, 1, 63, 64, 65, 700, 333]
    Q, KV8, _ = quantized(len(lens), H, N_q, 700, dtype, fmt, 3 * H)
    KV16 = KV8.to(dtype)
    assert torch.equal(KV16.float(), KV8.float())
    scale = 0.002 if fmt == E4 else 2e-5  # the raw cache values reach 448 / 57344
    for n in (1, 3, 16):
        for causal, window in ((True, None), (False, (100, 50))):
            kw = dict(causal=causal, scale=scale, window=window, num_splits=n, variant=variant)
            O, L = fa.flash_attention_mla_decode_forward(Q, KV8, lens_of(lens), DEV, **kw)
            O16, L16 = fa.flash_attention_mla_decode_forward(Q, KV16, lens_of(lens), DEV, **kw)
            assert not torch.isnan(O.float()).any() and same_bits(O, O16) and same_bits(L, L16), (dtype, fmt, variant, n, causal, window)


@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_every_finite_byte_is_staged_exactly(dtype, fmt, variant):
    """A cache that holds each finite byte pattern of the format, subnormals included, at every position of a 16-element load, in the
    first 512 columns and in the last 64: bit-identical to the 16-bit call on the converted cache."""
    B, H, N_q, S_k, d = 2, 16, 1, 320, 576
    b = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    b = b[torch.isfinite(b.view(fmt).float())]
    nb = b.numel()
    g = torch.Generator().manual_seed(nb)
    idx = torch.randint(0, nb, (B, 1, S_k, d), generator=g)
    idx.view(-1)[:17 * nb] = torch.arange(nb).repeat_interleave(17)          # every byte at every offset modulo 16 (576 % 16 == 0)
    idx[1, 0, :, 512:] = (torch.arange(S_k * 64) // 17 % nb).view(S_k, 64)   # ... and again in the last 64 columns (64 % 16 == 0)
    col = torch.arange(d).expand_as(idx)
    for region in (col < 512, col >= 512):
        pairs = torch.unique(idx[region] * 16 + col[region] % 16)
        assert pairs.numel() == 16 * nb
    KV8 = b[idx].to(DEV).view(fmt)
    Q = (torch.randn(B, H, N_q, d, generator=g) * 0.5).to(dtype).to(DEV)
    scale = 1e-3 if fmt == E4 else 1e-5
    for n in (1, 2):
        kw = dict(scale=scale, num_splits=n, variant=variant)
        O, L = fa.flash_attention_mla_decode_forward(Q, KV8, None, DEV, **kw)
        O16, L16 = fa.flash_attention_mla_decode_forward(Q, KV8.to(dtype), None, DEV, **kw)
        assert not torch.isnan(O.float()).any() and same_bits(O, O16) and same_bits(L, L16), (dtype, fmt, variant, n)


@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
def test_stale_rows_with_nan_and_inf_bytes_do_not_reach_the_output(fmt, variant):
    lens, H = [0, 1, 63, 64, 65, 1000, 300, 511], 40
    for N_q, causal, window, n in ((1, False, None, 0), (3, True, None, 1), (2, False, (100, 50), 4), (1, False, None, 128)):
        Q, KV8, kvd = quantized(len(lens), H, N_q, 1024, BF16, fmt, 5)
        outs = []
        for byte in (0,) + POISON:
            KVf = KV8.clone().view(torch.uint8)
            for b, nk in enumerate(lens):
                KVf[b, :, nk:] = byte
            outs.append(fa.flash_attention_mla_decode_forward(Q, KVf.view(fmt), lens_of(lens), DEV, causal=causal, window=window,
                                                              scale=0.1, num_splits=n, variant=variant, kv_descale=kvd))
        for O, L in outs[1:]:
            assert not torch.isnan(O).any() and not torch.isnan(L).any()
            assert same_bits(O, outs[0][0]) and same_bits(L, outs[0][1]), (fmt, variant, N_q, causal, window, n)


@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
@pytest.mark.parametrize("num_splits", [0, 1, 5])
def test_empty_rows_are_exact(variant, num_splits):
    lens, N_q, H = [0, 3, 10, 0], 5, 16
    Q, KV8, kvd = quantized(4, H, N_q, 256, BF16, E4, 3)
    O, L = fa.flash_attention_mla_decode_forward(Q, KV8, lens_of(lens), DEV, causal=True, num_splits=num_splits, variant=variant,
                                                 kv_descale=kvd, scale=SCALE)
    for b, rows in ((0, range(5)), (1, range(2)), (3, range(5))):
        for q in rows:
            assert (O[b, :, q] == 0).all() and torch.isinf(L[b, :, q]).all() and (L[b, :, q] > 0).all(), (b, q)
    assert torch.isfinite(L[1, :, 2:]).all() and torch.isfinite(L[2]).all()
    check_forward(O, L, *truth(Q, KV8, kvd, kvd, lens, True, SCALE, None), BF16, (variant, num_splits))


@pytest.mark.parametrize("fmt,variant", [(E4, "mla16"), (E5, "mla16"), (E4, "generic")], ids=ids)
def test_workspace_poison_determinism_and_canaries(fmt, variant):
    B, H, N_q, S_k = 5, 40, 2, 700
    lens = lens_of([0, 17, 700, 333, 64])
    Q, KV8, kvd = quantized(B, H, N_q, S_k, BF16, fmt, 9)
    V8 = KV8[..., :512]
    enum, kv_enum = convert_triton_dtype(BF16), convert_triton_dtype(fmt)
    kw = dict(k_descale=kvd, v_descale=kvd, causal=True, scale=0.1, variant=MLA[variant])
    for n in (4, 128):
        words = _lib.kvcache_workspace_bytes(B, H, N_q, 512, n) // 4
        results = []
        for poison in (0.0, float("nan"), float("nan")):
            O, O_all, O_sl = arena(B * H * N_q * 512, BF16, 77.0)
            L, L_all, L_sl = arena(B * H * N_q, BF16, 77.0)
            ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
            ws.fill_(poison)
            O4, L3 = O.view(B, H, N_q, 512), L.view(B, H, N_q)
            _lib.fa2_fwd_kvcache_mla_fp8(Q, KV8, V8, O4, L3, lens, enum, kv_enum, num_splits=n, workspace=ws, **kw)
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
            assert not torch.isnan(ws).any()  # every (split, row) partial was written
            results.append((O4.clone(), L3.clone()))
        for O4, L3 in results[1:]:  # NaN-poisoned == zeroed workspace, and the same call twice
            assert same_bits(O4, results[0][0]) and same_bits(L3, results[0][1]), (fmt, variant, n)
    # num_splits = 1: a poisoned workspace is neither read nor written; O and L inside their arenas
    O_ref, L_ref = fa.flash_attention_mla_decode_forward(Q, KV8, lens, DEV, causal=True, scale=0.1, num_splits=1, variant=variant,
                                                         kv_descale=kvd)
    ws, ws_all, ws_sl = arena(1000, torch.float32, 77.0)
    ws.fill_(float("nan"))
    O, O_all, O_sl = arena(B * H * N_q * 512, BF16, 77.0)
    L, L_all, L_sl = arena(B * H * N_q, BF16, 77.0)
    _lib.fa2_fwd_kvcache_mla_fp8(Q, KV8, V8, O.view(B, H, N_q, 512), L.view(B, H, N_q), lens, enum, kv_enum, num_splits=1, workspace=ws,
                                 **kw)
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and canaries_intact(ws_all, ws_sl, 77.0)
    assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0)
    assert same_bits(O.view(B, H, N_q, 512), O_ref) and same_bits(L.view(B, H, N_q), L_ref)


def scatter(KV8, page, seed):
    """(pool, table): the cache's pages, as bytes, under a seeded random permutation; three spare pages of the format's NaN byte"""
    fmt, raw = KV8.dtype, KV8.view(torch.uint8)
    B, h_kv, s_k, d = raw.shape
    mb = s_k // page
    assert mb * page == s_k
    nb = B * mb + 3
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:B * mb].view(B, mb)
    pool = torch.full((nb, h_kv, page, d), 0x7F, dtype=torch.uint8, device=DEV)
    pool[table.view(-1)] = raw.view(B, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(B * mb, h_kv, page, d)
    return pool.view(fmt), table.to(torch.int32).contiguous()


@pytest.mark.parametrize("dtype,fmt,variant,page", [(BF16, E4, "mla16", 64), (F16, E5, "mla16", 128), (BF16, E5, "generic", 16),
                                                    (F16, E4, "generic", 16)], ids=ids)
def test_paged_equals_contiguous_bit_for_bit(dtype, fmt, variant, page):
    H, lens = 72, [0, 1, 64, 65, 700, 1280]
    for N_q, causal, window, n in ((1, False, None, 0), (2, True, None, 1), (2, False, (100, 50), 5)):
        Q, KV8, kvd = quantized(len(lens), H, N_q, 1280, dtype, fmt, 13)
        pool, table = scatter(KV8, page, page + N_q)
        kw = dict(causal=causal, window=window, scale=SCALE, num_splits=n, variant=variant, kv_descale=kvd)
        O, L = fa.flash_attention_mla_decode_forward(Q, KV8, lens_of(lens), DEV, **kw)
        Op, Lp = fa.flash_attention_mla_decode_forward(Q, pool, lens_of(lens), DEV, block_table=table, **kw)
        assert not torch.isnan(Op).any() and same_bits(Op, O) and same_bits(Lp, L), (N_q, causal, window, n)
    # "auto" takes the VALU form where the page size is no multiple of 64, a forced matrix form refuses it
    if page == 16:
        Oa, La = fa.flash_attention_mla_decode_forward(Q, pool, lens_of(lens), DEV, block_table=table, **dict(kw, variant="auto"))
        assert same_bits(Oa, Op) and same_bits(La, Lp)
        with pytest.raises(TypeError, match="page_size % 64"):
            fa.flash_attention_mla_decode_forward(Q, pool, lens_of(lens), DEV, block_table=table, **dict(kw, variant="mla16"))


@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
@pytest.mark.parametrize("d,d_v", [(576, 512), (192, 128)])
def test_separate_v_on_the_valu_form(fmt, d, d_v):
    """V a tensor of its own, quantised on its own: the generic kernel, which AUTO takes and a forced matrix form refuses; and the
    (192, 128) view through the convenience function"""
    H, N_q, lens = 16, 2, [0, 65, 300, 1000]
    dtype = BF16 if fmt == E4 else F16
    Q, K8, kd = quantized(len(lens), H, N_q, 1000, dtype, fmt, d, d=d)
    V = (torch.randn(len(lens), 1, 1000, d_v, generator=torch.Generator().manual_seed(d_v)) * 0.5).to(dtype).to(DEV)
    V8, vd = fa.quantize_kv_cache(V, fmt)
    for n, causal, window in ((1, True, None), (3, False, (100, 50)), (0, False, None)):
        ref = truth(Q, K8, kd, vd, lens, causal, d ** -0.5, window, V8=V8)
        for variant in ("generic", "auto"):
            O, L = launch(Q, K8, V8, lens_of(lens), kd, vd, variant, n, causal=causal, scale=d ** -0.5, window=window)
            check_forward(O, L, *ref, dtype, (fmt, d, d_v, variant, n, causal, window))
        if d != 576:
            O, L = fa.flash_attention_mla_decode_forward(Q, K8, lens_of(lens), DEV, d_v=d_v, causal=causal, scale=d ** -0.5,
                                                         window=window, num_splits=n, kv_descale=kd)
            check_forward(O, L, *truth(Q, K8, kd, kd, lens, causal, d ** -0.5, window, d_v=d_v), dtype, (fmt, "view", d, d_v, n))
    with pytest.raises(TypeError, match="aliasing"):  # FA2_ERR_UNSUPPORTED
        launch(Q, K8, V8, lens_of(lens), kd, vd, "mla16", 1)


@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
def test_two_descales_on_the_shared_row_are_independent(fmt, variant):
    """K and V are the same bytes, k_descale and v_descale still two scalars: any pair, also one of them null.  (The rows are stored
    at their own magnitude, rounded to fp8, so that O stays of order 1 -- where the absolute bar is meant -- under a null descale.)"""
    lens, H, N_q = [700, 129, 5], 16, 2
    Q, KV = make(len(lens), H, N_q, 700, BF16, 29)
    KV8 = KV.to(fmt)
    one, other = torch.tensor([[1.7], [0.6], [1.3]], device=DEV), torch.tensor([[0.45], [2.1], [0.9]], device=DEV)
    for kd, vd in ((one, other), (other, one), (one, None), (None, other)):
        for n in (1, 3):
            O, L = launch(Q, KV8, KV8[..., :512], lens_of(lens), kd, vd, variant, n, causal=True, scale=0.05)
            check_forward(O, L, *truth(Q, KV8, kd, vd, lens, True, 0.05, None), BF16, (fmt, variant, n, kd is None, vd is None))


@pytest.mark.parametrize("variant", ["mla16", "generic"])
@pytest.mark.parametrize("fmt", [E4, E5], ids=ids)
def test_kv_descale_broadcasting(fmt, variant):
    B, H, H_kv, N_q, S_k = 3, 16, 2, 2, 600
    Q, KV8, kvd = quantized(B, H, N_q, S_k, BF16, fmt, 17, H_kv=H_kv)
    lens = lens_of([600, 129, 5])
    full = lambda t: torch.broadcast_to(t, (B, H_kv)).contiguous()
    scalar = torch.tensor(0.37, device=DEV)                        # 0-d
    col = kvd[:, :1].contiguous()                                  # (B, 1)
    row = kvd[:1].contiguous()                                     # (1, H_kv)
    transposed = kvd.t().contiguous().t()                          # (B, H_kv) with strides (1, B)
    assert kvd.shape == (B, H_kv) and transposed.stride() == (1, B)
    pairs = [(None, torch.ones(B, H_kv, device=DEV)), (scalar, full(scalar)), (col, full(col)), (row, full(row)), (kvd[0], full(kvd[0])),
             (transposed, kvd)]
    for n in (1, 3):
        call = lambda t: fa.flash_attention_mla_decode_forward(Q, KV8, lens, DEV, causal=True, scale=0.05, num_splits=n, variant=variant,
                                                               kv_descale=t)
        results = []
        for short, explicit in pairs:
            (O, L), (Oe, Le) = call(short), call(explicit)
            assert same_bits(O, Oe) and same_bits(L, Le), (fmt, variant, n, None if short is None else tuple(short.shape))
            results.append(O)
        assert not torch.equal(results[2], results[3])             # ... and do reach the result
        check_forward(*call(kvd), *truth(Q, KV8, kvd, kvd, [600, 129, 5], True, 0.05, None), BF16, (fmt, variant, n))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
def test_sixteen_bit_cache_through_the_new_entry_point(dtype, variant):
    """fa2_fwd_kvcache_mla_fp8 with kv_dtype_enum == dtype_enum and null descales gives the bits of fa2_fwd_kvcache_mla"""
    lens, H, N_q = [5, 300, 777, 0], 40, 2
    Q, KV = make(len(lens), H, N_q, 777, dtype, 17)
    for n in (0, 1, 4):
        for causal, window in ((True, None), (False, (100, 50))):
            O, L = launch(Q, KV, KV[..., :512], lens_of(lens), None, None, variant, n, causal=causal, window=window,
                          kv_enum=convert_triton_dtype(dtype))
            Oe, Le = fa.flash_attention_mla_decode_forward(Q, KV, lens_of(lens), DEV, causal=causal, window=window, scale=SCALE,
                                                           num_splits=n, variant=variant)
            assert same_bits(O, Oe) and same_bits(L, Le), (dtype, variant, n, causal, window)
    with pytest.raises(ValueError, match="go with an fp8"):      # descales with a 16-bit cache: FA2_ERR_BAD_ARG
        launch(Q, KV, KV[..., :512], lens_of(lens), torch.ones(1, device=DEV), None, variant, 1, kv_enum=convert_triton_dtype(dtype))
