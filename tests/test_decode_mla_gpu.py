"""MLA decode (fa2_fwd_kvcache_mla) on the GPU with random data: O and L against the fp64 per-sequence truth for every variant and
dtype, an aliased and a separate V, stale rows and a poisoned workspace that must not reach the output, canary arenas, paged
against contiguous bit for bit, the convenience function against the explicit view, and the d = 128 path left as it was.  The bars
are those of tests/test_decode_gpu.py, imported: O_TOL, for L 1.01 ulp on 16-bit I/O and 5e-5 relative on float32 / float64."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_bwd_arith
from test_decode_gpu import arena, canaries_intact, check_forward, f32, lens_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
S_K = 2560
LENS = [0, 1, 63, 64, 65, 1000, 2049, S_K]
SPLITS = (0, 1, 3, 16, 128)
SCALE = 576 ** -0.5


def make(B, H, N_q, S_k, dtype, seed, d=576, H_kv=1, amp=0.5):
    g = torch.Generator().manual_seed(seed)
    Q = (torch.randn(B, H, N_q, d, generator=g) * amp).to(dtype).to(DEV)
    KV = (torch.randn(B, H_kv, S_k, d, generator=g) * amp).to(dtype).to(DEV)
    return Q, KV


def reference(Q, K, V, lens, causal, scale, window):
    """tests/test_decode_gpu.py's reference() for a V of its own width: the fp64 truth, one sequence at a time (every head of it at
    once), over the first N_k(b) keys: O (B, H, N_q, d_v), L (B, H, N_q); rows without a visible key get O = 0 and L = +inf"""
    B, H, N_q, d = Q.shape
    H_kv, S_k, d_v = K.shape[1], K.shape[2], V.shape[3]
    g = H // H_kv
    O = torch.zeros(B, H, N_q, d_v, dtype=torch.float64, device=DEV)
    L = torch.full((B, H, N_q), math.inf, dtype=torch.float64, device=DEV)
    for b in range(B):
        nk = S_k if lens is None else min(max(int(lens[b]), 0), S_k)
        m = fa2_bwd_arith.band(N_q, nk, causal, window, DEV)
        vis = m.any(-1)
        q, k, v = Q[b].double().view(H_kv, g, N_q, d), K[b, :, :nk].double(), V[b, :, :nk].double()
        S = torch.einsum("kgqd,knd->kgqn", q, k) * f32(scale)
        S = S.masked_fill(~m, float("-inf"))
        P = torch.where(vis.view(N_q, 1), torch.softmax(S.masked_fill(~vis.view(N_q, 1), 0.0), -1), 0.0)
        O[b] = torch.einsum("kgqn,knd->kgqd", P, v).reshape(H, N_q, d_v)
        L[b] = torch.where(vis, torch.logsumexp(S, -1) * math.log2(math.e), math.inf).reshape(H, N_q)
    return O, L


_TRUTH = {}


def truth(H, N_q, causal, dtype):
    """Q, KV and the fp64 truth of one shape: computed once, shared by the variants and split counts, never modified"""
    key = (H, N_q, causal, dtype)
    if key not in _TRUTH:
        Q, KV = make(len(LENS), H, N_q, S_K, dtype, 11 * H + N_q)
        _TRUTH[key] = (Q, KV) + reference(Q, KV, KV[..., :512], LENS, causal, SCALE, None)
    return _TRUTH[key]


CASES = [(dt, v) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")] + [(F32, "generic"), (F64, "generic")]


@pytest.mark.parametrize("H,N_q", [(16, 1), (16, 2), (128, 1), (128, 2)])
@pytest.mark.parametrize("dtype,variant", CASES)
def test_forward_against_fp64_truth(dtype, variant, H, N_q):
    lens = lens_of(LENS)
    for causal in (False, True):
        Q, KV, O_ref, L_ref = truth(H, N_q, causal, dtype)
        for n in SPLITS:
            O, L = fa.flash_attention_mla_decode_forward(Q, KV, lens, DEV, causal=causal, scale=SCALE, num_splits=n, variant=variant)
            assert O.shape == (len(LENS), H, N_q, 512) and L.shape == (len(LENS), H, N_q) and O.dtype == dtype and L.dtype == dtype
            check_forward(O, L, O_ref, L_ref, dtype, (dtype, variant, H, N_q, causal, n))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("d,d_v", [(576, 512), (192, 128)])
def test_separate_v_on_the_valu_form(dtype, d, d_v):
    """V a tensor of its own: the generic kernel, which AUTO takes and a forced matrix form refuses"""
    H, N_q = 16, 2
    lens = [0, 65, 300, 1000]
    Q, K = make(len(lens), H, N_q, 1000, dtype, d, d=d)
    V = (torch.randn(len(lens), 1, 1000, d_v, generator=torch.Generator().manual_seed(d_v)) * 0.5).to(dtype).to(DEV)
    for n, causal, window in ((1, True, None), (3, False, (100, 50)), (0, False, None)):
        O_ref, L_ref = reference(Q, K, V, lens, causal, d ** -0.5, window)
        for variant in ("generic", "auto"):
            O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, causal=causal, scale=d ** -0.5, window=window,
                                                      num_splits=n, variant=variant)
            assert O.shape == (len(lens), H, N_q, d_v)
            check_forward(O, L, O_ref, L_ref, dtype, (dtype, d, d_v, variant, n, causal, window))
    with pytest.raises(TypeError):  # FA2_ERR_UNSUPPORTED
        fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, variant="mla16")


@pytest.mark.parametrize("dtype,variant", [(BF16, "mla16"), (F16, "auto"), (BF16, "generic"), (F32, "generic")])
def test_stale_rows_do_not_reach_the_output(dtype, variant):
    lens, H = [0, 1, 63, 64, 65, 1000, 300, 511], 40
    for N_q, causal, window, n in ((1, False, None, 0), (3, True, None, 1), (2, False, (100, 50), 4), (1, False, None, 128)):
        Q, KV = make(len(lens), H, N_q, 1024, dtype, 5)
        outs = []
        for fill in (0.0, float("nan"), float("inf"), float("-inf")):
            KVf = KV.clone()
            for b, nk in enumerate(lens):
                KVf[b, :, nk:] = fill
            outs.append(fa.flash_attention_mla_decode_forward(Q, KVf, lens_of(lens), DEV, causal=causal, window=window, scale=0.1,
                                                              num_splits=n, variant=variant))
        for O, L in outs[1:]:
            assert not torch.isnan(O).any() and not torch.isnan(L).any()
            assert torch.equal(O, outs[0][0]) and torch.equal(L, outs[0][1]), (N_q, causal, window, n)


@pytest.mark.parametrize("dtype,variant", [(BF16, "mla16"), (BF16, "generic"), (F32, "generic")])
def test_workspace_poison_determinism_and_canaries(dtype, variant):
    B, H, N_q, S_k = 5, 40, 2, 700
    lens = lens_of([0, 17, 700, 333, 64])
    Q, KV = make(B, H, N_q, S_k, dtype, 9)
    V = KV[..., :512]
    enum = convert_triton_dtype(dtype)
    for n in (4, 128):
        words = _lib.kvcache_workspace_bytes(B, H, N_q, 512, n) // 4
        results = []
        for poison in (0.0, float("nan"), float("nan")):
            O, O_all, O_sl = arena(B * H * N_q * 512, dtype, 77.0)
            L, L_all, L_sl = arena(B * H * N_q, dtype, 77.0)
            ws, ws_all, ws_sl = arena(words, torch.float32, 77.0)
            ws.fill_(poison)
            O4, L3 = O.view(B, H, N_q, 512), L.view(B, H, N_q)
            _lib.fa2_fwd_kvcache_mla(Q, KV, V, O4, L3, lens, enum, causal=True, scale=0.1, num_splits=n, workspace=ws,
                                     variant=_lib.KVCACHE_MLA_VARIANTS[variant])
            torch.cuda.synchronize()
            assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0) and canaries_intact(ws_all, ws_sl, 77.0)
            assert not torch.isnan(ws).any()  # every (split, row) partial was written
            results.append((O4.clone(), L3.clone()))
        for O4, L3 in results[1:]:  # NaN-poisoned == zeroed workspace, and the same call twice
            assert torch.equal(O4, results[0][0]) and torch.equal(L3, results[0][1]), (variant, n)
    # num_splits = 1: a poisoned workspace is neither read nor written; O and L inside their arenas
    O_ref, L_ref = fa.flash_attention_mla_decode_forward(Q, KV, lens, DEV, causal=True, scale=0.1, num_splits=1, variant=variant)
    ws, ws_all, ws_sl = arena(1000, torch.float32, 77.0)
    ws.fill_(float("nan"))
    O, O_all, O_sl = arena(B * H * N_q * 512, dtype, 77.0)
    L, L_all, L_sl = arena(B * H * N_q, dtype, 77.0)
    _lib.fa2_fwd_kvcache_mla(Q, KV, V, O.view(B, H, N_q, 512), L.view(B, H, N_q), lens, enum, causal=True, scale=0.1, num_splits=1,
                             workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and canaries_intact(ws_all, ws_sl, 77.0)
    assert canaries_intact(O_all, O_sl, 77.0) and canaries_intact(L_all, L_sl, 77.0)
    assert torch.equal(O.view(B, H, N_q, 512), O_ref) and torch.equal(L.view(B, H, N_q), L_ref)


def scatter(KV, page, seed):
    """(pool, table): the cache's pages under a seeded random permutation, three spare pages of NaN"""
    B, h_kv, s_k, d = KV.shape
    mb = s_k // page
    assert mb * page == s_k
    nb = B * mb + 3
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(DEV)
    table = perm[:B * mb].view(B, mb)
    pool = torch.full((nb, h_kv, page, d), float("nan"), dtype=KV.dtype, device=DEV)
    pool[table.view(-1)] = KV.view(B, h_kv, mb, page, d).permute(0, 2, 1, 3, 4).reshape(B * mb, h_kv, page, d)
    return pool, table.to(torch.int32).contiguous()


@pytest.mark.parametrize("dtype,variant,page", [(BF16, "mla16", 64), (F16, "mla16", 128), (BF16, "generic", 16), (F32, "generic", 16)])
def test_paged_equals_contiguous_bit_for_bit(dtype, variant, page):
    H, lens = 72, [0, 1, 64, 65, 700, 1280]
    for N_q, causal, window, n in ((1, False, None, 0), (2, True, None, 1), (2, False, (100, 50), 5)):
        Q, KV = make(len(lens), H, N_q, 1280, dtype, 13)
        pool, table = scatter(KV, page, page + N_q)
        kw = dict(causal=causal, window=window, scale=SCALE, num_splits=n, variant=variant)
        O, L = fa.flash_attention_mla_decode_forward(Q, KV, lens_of(lens), DEV, **kw)
        Op, Lp = fa.flash_attention_mla_decode_forward(Q, pool, lens_of(lens), DEV, block_table=table, **kw)
        assert not torch.isnan(Op).any() and torch.equal(Op, O) and torch.equal(Lp, L), (N_q, causal, window, n)
    # "auto" takes the VALU form where the page size is no multiple of 64, a forced matrix form refuses it
    if page == 16 and dtype == BF16:
        Oa, La = fa.flash_attention_mla_decode_forward(Q, pool, lens_of(lens), DEV, block_table=table, **dict(kw, variant="auto"))
        assert torch.equal(Oa, Op) and torch.equal(La, Lp)
        with pytest.raises(TypeError):
            fa.flash_attention_mla_decode_forward(Q, pool, lens_of(lens), DEV, block_table=table, **dict(kw, variant="mla16"))


@pytest.mark.parametrize("variant", ["auto", "mla16", "generic"])
def test_convenience_function_is_the_explicit_view_call(variant):
    lens, H, N_q = [5, 300, 777], 16, 2
    Q, KV = make(len(lens), H, N_q, 777, BF16, 17)
    for n in (0, 1, 4):
        kw = dict(causal=True, scale=SCALE, num_splits=n, variant=variant)
        O, L = fa.flash_attention_mla_decode_forward(Q, KV, lens_of(lens), DEV, **kw)
        Oe, Le = fa.flash_attention_kvcache_forward(Q, KV, KV[..., :512], lens_of(lens), DEV, **kw)
        assert torch.equal(O, Oe) and torch.equal(L, Le)
    # another d_v: columns 0..127 of a 192-wide row, the VALU form
    Q2, KV2 = make(len(lens), H, N_q, 777, BF16, 19, d=192)
    if variant != "mla16":
        O, L = fa.flash_attention_mla_decode_forward(Q2, KV2, lens_of(lens), DEV, d_v=128, scale=0.1, variant=variant)
        check_forward(O, L, *reference(Q2, KV2, KV2[..., :128], lens, False, 0.1, None), BF16, ("d_v 128", variant))


def test_layouts_and_h_kv_above_one():
    """a (B, S, H_kv, d) latent cache and a (B, N_q, H, d) query viewed head-first, two KV heads: strides, not copies"""
    B, H, H_kv, N_q, S = 3, 80, 2, 1, 600
    lens = [600, 129, 5]
    Q, KV = make(B, H, N_q, S, BF16, 23, H_kv=H_kv)
    bshd = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    O_ref, L_ref = reference(Q, KV, KV[..., :512], lens, False, SCALE, None)
    for variant in ("mla16", "generic"):
        for n in (1, 3):
            O, L = fa.flash_attention_mla_decode_forward(bshd(Q), bshd(KV), lens_of(lens), DEV, scale=SCALE, num_splits=n, variant=variant)
            check_forward(O, L, O_ref, L_ref, BF16, ("bshd", variant, n))


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_d_128_path_is_unchanged(dtype):
    """equal shapes take today's path: generic and mfma16 against each other and the truth, as tests/test_decode_gpu.py does; the
    generic kernel run through the new entry point with d_v == d gives the old entry point's bits"""
    B, H, H_kv, N_q, S, d = 4, 8, 2, 2, 700, 128
    lens = [0, 65, 300, 700]
    g = torch.Generator().manual_seed(31)
    Q = (torch.randn(B, H, N_q, d, generator=g) * 0.5).to(dtype).to(DEV)
    K = (torch.randn(B, H_kv, S, d, generator=g) * 0.5).to(dtype).to(DEV)
    V = (torch.randn(B, H_kv, S, d, generator=g) * 0.5).to(dtype).to(DEV)
    enum = convert_triton_dtype(dtype)
    for n in (1, 3):
        O_ref, L_ref = reference(Q, K, V, lens, True, 0.09, None)
        outs = {}
        for variant in ("generic", "auto") + (("mfma16",) if dtype != F32 else ()):
            outs[variant] = fa.flash_attention_kvcache_forward(Q, K, V, lens_of(lens), DEV, causal=True, scale=0.09, num_splits=n,
                                                               variant=variant)
            assert outs[variant][0].shape == Q.shape
            check_forward(*outs[variant], O_ref, L_ref, dtype, ("d 128", dtype, variant, n))
        if dtype != F32:  # auto is the matrix form, bit for bit
            assert torch.equal(outs["auto"][0], outs["mfma16"][0]) and torch.equal(outs["auto"][1], outs["mfma16"][1])
        # the same VALU kernel through fa2_fwd_kvcache_mla with d_v == d: the bits of the old entry point
        O, L = torch.empty_like(outs["generic"][0]), torch.empty_like(outs["generic"][1])
        ws = torch.empty(_lib.kvcache_workspace_bytes(B, H, N_q, d, n) // 4, dtype=torch.float32, device=DEV) if n > 1 else None
        _lib.fa2_fwd_kvcache_mla(Q, K, V, O, L, lens_of(lens), enum, causal=True, scale=0.09, num_splits=n, workspace=ws,
                                 variant=_lib.KVCACHE_MLA_VARIANTS["generic"])
        assert torch.equal(O, outs["generic"][0]) and torch.equal(L, outs["generic"][1])
