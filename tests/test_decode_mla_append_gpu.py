"""The latent-cache append on the GPU (fa2_kvcache_mla_append, fa2_kvcache_mla_append_varlen, fa2_fwd_kvcache_mla_append).  The
yardstick is tests/mla_append_restatement.py on the CPU; caches start as random bytes and are compared WHOLE through integer views,
so a stray write anywhere fails.  Every comparison is an equality of bits: the arithmetic is pinned (fp32, every product and sum
rounded on its own, one rounding to the cache's dtype), and the fused call runs the same kernels as the two calls it replaces."""
import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from decode_append_restatement import bits
from mla_append_restatement import expected_mla_append, expected_mla_append_packed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, S_K, PAGE, S_ROT = 3, 16, 192, 64, 100        # S_ROT < the largest position: the position clamp
LENS = [0, 63, 190]                                 # a page crossing (63 -> 64) and, with 3 tokens, one dropped (192 = capacity)
LENS_CLAMPS = [-5, 64, 500]                         # clamped to 0 and to the capacity
# 7 pages of 64 rows; entry 99 is out of range (clamped to page 6, which sequence 2 writes), page 1 is shared and only read
TABLE = [[0, 1, 1], [2, 3, 1], [4, 5, 99]]
F8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def _random_bytes(shape, dtype, g):
    n = torch.empty(shape, dtype=dtype)
    raw = torch.randint(0, 256, (n.numel() * n.element_size(),), dtype=torch.uint8, generator=g)
    return raw.view(dtype).view(shape)


def _tables(rd, dtype, g):
    ang = torch.rand(S_ROT, rd // 2, generator=g, dtype=torch.float64) * 6.283
    return ang.cos().to(dtype), ang.sin().to(dtype)


class Problem:
    def __init__(self, dtype, cache_dtype=None, H_kv=1, n_new=1, paged=False, lens=LENS, rd=64, d=576, d_v=512, seed=0, finite=False,
                 saturate=False):
        g = torch.Generator().manual_seed(seed)
        self.d, self.d_v, self.paged, self.H_kv = d, d_v, paged, H_kv
        cache_dtype = cache_dtype or dtype
        shape = (7, H_kv, PAGE, d) if paged else (B, H_kv, S_K, d)
        if finite:  # a cache an attention can read
            self.KV0 = (torch.randn(shape, generator=g) * 0.5).to(dtype).to(cache_dtype)
        else:
            self.KV0 = _random_bytes(shape, cache_dtype, g)
        self.table = torch.tensor(TABLE, dtype=torch.int32) if paged else None
        self.c = torch.randn(B, H_kv, n_new, d_v, generator=g).to(dtype)
        self.pe = torch.randn(B, H_kv, n_new, d - d_v, generator=g).to(dtype)
        if saturate:  # beyond +-max of either fp8 format after the division
            self.c[..., 0:4] = torch.tensor([60000.0, -60000.0, 30000.0, -448.0]).to(dtype)
            self.pe[..., 1] = -60000.0
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.cos, self.sin = _tables(rd, dtype, g) if rd else (None, None)
        self.descale = (0.37 + 0.11 * torch.arange(B * H_kv, dtype=torch.float32).view(B, H_kv)) if cache_dtype in F8 else None

    def expected(self, interleaved=False):
        return expected_mla_append(self.KV0, self.c, self.pe, self.lens, self.d_v, self.table, self.descale, self.cos, self.sin, interleaved)


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(p, kv_new=None, interleaved=False):
    """mla_kvcache_append on device copies -> (KV after, new_seqlens), both on the CPU; the lengths must come out unchanged."""
    KV, lens = p.KV0.to(DEV), p.lens.to(DEV)
    kv_new = (p.c.to(DEV), p.pe.to(DEV)) if kv_new is None else kv_new
    got = fa.mla_kvcache_append(KV, kv_new, lens, d_v=p.d_v, kv_descale=_dev(p.descale), block_table=_dev(p.table),
                                rotary_cos=_dev(p.cos), rotary_sin=_dev(p.sin), rotary_interleaved=interleaved)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and torch.equal(lens.cpu(), p.lens)
    return KV.cpu(), got.cpu()


def _same(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("dtype,H_kv,n_new,paged,lens,rd,interleaved,d,d_v", [
    (torch.bfloat16, 1, 1, False, LENS, 64, False, 576, 512),
    (torch.bfloat16, 2, 3, True, LENS, 64, True, 576, 512),
    (torch.float16, 2, 3, True, LENS, 32, False, 576, 512),          # a pass-through tail behind the rotary range
    (torch.float16, 1, 3, False, LENS_CLAMPS, 32, True, 576, 512),
    (torch.bfloat16, 1, 3, True, LENS_CLAMPS, 64, False, 576, 512),
    (torch.bfloat16, 2, 3, True, LENS, 0, False, 576, 512),          # no rotary at all
    (torch.float32, 2, 3, True, LENS, 64, False, 192, 128),          # the element path
    (torch.float32, 1, 1, False, LENS_CLAMPS, 32, True, 192, 128),
    (torch.float64, 2, 3, False, LENS, 32, False, 192, 128),
])
def test_cache_bytes_equal_the_restatement(dtype, H_kv, n_new, paged, lens, rd, interleaved, d, d_v):
    p = Problem(dtype, H_kv=H_kv, n_new=n_new, paged=paged, lens=lens, rd=rd, d=d, d_v=d_v, seed=1)
    want, _, want_len = p.expected(interleaved)
    got, got_len = _run(p, interleaved=interleaved)
    assert not _same(want, p.KV0)
    assert torch.equal(got_len, want_len), (got_len, want_len)
    assert _same(got, want), f"{(bits(got) != bits(want)).sum().item()} elements differ"


@pytest.mark.parametrize("cache_dtype", F8)
@pytest.mark.parametrize("dtype,H_kv,n_new,paged,rd,interleaved", [
    (torch.bfloat16, 2, 3, True, 64, False), (torch.float16, 1, 1, False, 32, True), (torch.float16, 2, 3, False, 0, False)])
def test_fp8_cache_with_descales_and_saturation(cache_dtype, dtype, H_kv, n_new, paged, rd, interleaved):
    p = Problem(dtype, cache_dtype, H_kv=H_kv, n_new=n_new, paged=paged, rd=rd, seed=2, saturate=True)
    want, _, want_len = p.expected(interleaved)
    got, got_len = _run(p, interleaved=interleaved)
    top = torch.finfo(cache_dtype).max
    stored = want[0, 0, 0] if not paged else want[TABLE[0][0], 0, 0]     # sequence 0, token 0 sits at key 0
    assert stored[0].float() == top and stored[1].float() == -top   # saturated, not inf / NaN
    assert torch.equal(got_len, want_len)
    assert _same(got, want), f"{(bits(got) != bits(want)).sum().item()} bytes differ"


@pytest.mark.parametrize("cache_dtype", [None, torch.float8_e4m3fn])
@pytest.mark.parametrize("interleaved", [False, True])
def test_one_tensor_the_pair_and_the_element_path_give_the_same_bytes(cache_dtype, interleaved):
    p = Problem(torch.bfloat16, cache_dtype, H_kv=2, n_new=3, paged=True, seed=3)
    want, _, _ = p.expected(interleaved)
    pair, _ = _run(p, interleaved=interleaved)                                             # two allocations: the vector path
    assert _same(pair, want)
    one, _ = _run(p, torch.cat([p.c, p.pe], dim=-1).to(DEV), interleaved)                  # one (..., 576) tensor
    assert _same(one, pair)
    c, pe = p.c.to(DEV), p.pe.to(DEV)
    wide = torch.zeros(*pe.shape[:3], 2 * pe.shape[3], dtype=pe.dtype, device=DEV)[..., ::2]
    wide.copy_(pe)                                                                         # a column stride of 2: the element path
    assert wide.stride(3) == 2 and _same(_run(p, (c, wide), interleaved)[0], pair)
    odd = torch.zeros(c.numel() + 1, dtype=c.dtype, device=DEV)[1:].view(c.shape)
    odd.copy_(c)                                                                           # misaligned by one element
    assert odd.data_ptr() % 16 == 2 and _same(_run(p, (odd, pe), interleaved)[0], pair)


CU, MAX_NEW, LENS4 = [0, 1, 1, 5, 6], 3, [63, 5, 190, 0]   # an empty sequence, a span of 4 capped at 3, and row 6 in no sequence
TABLE4 = TABLE + [[3, 1, 1]]


@pytest.mark.parametrize("cache_dtype,paged,rd,interleaved", [(None, False, 64, False), (None, True, 32, True), (torch.float8_e4m3fn, True, 64, False),
                                                              (torch.float8_e5m2, False, 0, False)])
def test_packed_form(cache_dtype, paged, rd, interleaved):
    dtype, H_kv, d, d_v, nb = torch.bfloat16, 2, 576, 512, 4
    g = torch.Generator().manual_seed(4)
    KV0 = _random_bytes((7, H_kv, PAGE, d) if paged else (nb, H_kv, S_K, d), cache_dtype or dtype, g)
    table = torch.tensor(TABLE4, dtype=torch.int32) if paged else None
    c, pe = torch.randn(7, H_kv, d_v, generator=g).to(dtype), torch.randn(7, H_kv, d - d_v, generator=g).to(dtype)
    cu, lens = torch.tensor(CU, dtype=torch.int32), torch.tensor(LENS4, dtype=torch.int32)
    cos, sin = _tables(rd, dtype, g) if rd else (None, None)
    descale = (0.29 + 0.07 * torch.arange(nb * H_kv, dtype=torch.float32).view(nb, H_kv)) if cache_dtype else None
    want, want_len = expected_mla_append_packed(KV0, c, pe, cu, MAX_NEW, lens, d_v, table, descale, cos, sin, interleaved)
    assert want_len.tolist() == [64, 5, 192, 1]
    kw = dict(d_v=d_v, rotary_cos=_dev(cos), rotary_sin=_dev(sin), rotary_interleaved=interleaved)
    KV, lens_d = KV0.to(DEV), lens.to(DEV)
    got_len = fa.mla_kvcache_append_varlen(KV, (c.to(DEV), pe.to(DEV)), cu.to(DEV), MAX_NEW, lens_d, kv_descale=_dev(descale),
                                           block_table=_dev(table), **kw)
    torch.cuda.synchronize()
    assert torch.equal(lens_d.cpu(), lens) and torch.equal(got_len.cpu(), want_len)          # the empty sequence's length too
    assert _same(KV.cpu(), want), f"{(bits(KV.cpu()) != bits(want)).sum().item()} elements differ"
    # ... and the fixed call, sequence by sequence
    KV2 = KV0.to(DEV)
    for b in range(nb):
        s, n = CU[b], min(CU[b + 1] - CU[b], MAX_NEW)
        if n == 0:
            continue
        fixed = lambda x: x[s:s + n].transpose(0, 1).unsqueeze(0).to(DEV)
        new = fa.mla_kvcache_append(KV2 if paged else KV2[b:b + 1], (fixed(c), fixed(pe)), lens_d[b:b + 1],
                                    kv_descale=None if descale is None else descale[b:b + 1].to(DEV),
                                    block_table=None if table is None else table[b:b + 1].to(DEV), **kw)
        assert new.cpu().tolist() == [want_len[b].item()]
    assert _same(KV2.cpu(), KV.cpu())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("cache_dtype", [None, torch.float8_e4m3fn])
def test_fused_call_equals_append_then_decode(cache_dtype, paged, causal, n):
    """O, L, the cache and the lengths of the fused step against mla_kvcache_append followed by the decode call on a Q whose last 64
    columns apply_rotary rotated at the documented positions: cache_seqlens[b] + i for row i when causal, cache_seqlens[b] otherwise."""
    dtype = torch.bfloat16
    p = Problem(dtype, cache_dtype, H_kv=1, n_new=n, paged=paged, seed=5 + n, finite=True)
    g = torch.Generator().manual_seed(9)
    Q = torch.randn(B, H, n, p.d, generator=g).to(dtype)
    cos, sin, table, descale = _dev(p.cos), _dev(p.sin), _dev(p.table), _dev(p.descale)
    common = dict(d_v=p.d_v, causal=causal, scale=p.d ** -0.5, block_table=table, kv_descale=descale)
    # the fused step
    KV1, lens = p.KV0.to(DEV), p.lens.to(DEV)
    O1, L1 = fa.flash_attention_mla_decode_forward(Q.to(DEV), KV1, lens, DEV, kv_new=(p.c.to(DEV), p.pe.to(DEV)), rotary_cos=cos,
                                                   rotary_sin=sin, **common)
    # the two calls
    KV2 = p.KV0.to(DEV)
    new = fa.mla_kvcache_append(KV2, (p.c.to(DEV), p.pe.to(DEV)), lens, d_v=p.d_v, kv_descale=descale, block_table=table, rotary_cos=cos,
                                rotary_sin=sin)
    pos = p.lens.long()[:, None, None] + (torch.arange(n)[None, None, :] if causal else 0)
    Qr = Q.clone()
    Qr[..., p.d_v:] = fa.apply_rotary(Q[..., p.d_v:], p.cos, p.sin, pos)
    O2, L2 = fa.flash_attention_mla_decode_forward(Qr.to(DEV), KV2, new, DEV, **common)
    # the lengths the fused step hands its attention: the entry point itself, single split
    KV3, out = p.KV0.to(DEV), torch.full_like(lens, -1)
    O3 = torch.empty(B, H, n, p.d_v, dtype=dtype, device=DEV)
    L3 = torch.empty(B, H, n, dtype=dtype, device=DEV)
    _lib.fa2_fwd_kvcache_mla_append(Q.to(DEV), KV3, O3, L3, p.c.to(DEV), p.pe.to(DEV), lens, out, convert_triton_dtype(dtype),
                                    convert_triton_dtype(KV3.dtype), block_table=table,
                                    kv_descale=None if descale is None else torch.broadcast_to(descale, (B, 1)), rotary_cos=cos,
                                    rotary_sin=sin, q_rot=torch.empty(B, H, n, p.d, dtype=dtype, device=DEV), causal=causal,
                                    scale=p.d ** -0.5, num_splits=1)
    torch.cuda.synchronize()
    want, _, want_len = p.expected()
    assert torch.equal(lens.cpu(), p.lens) and torch.equal(new.cpu(), want_len) and torch.equal(out.cpu(), want_len)
    assert _same(KV1.cpu(), want) and _same(KV2.cpu(), want) and _same(KV3.cpu(), want)
    assert torch.isfinite(O1.float()).all()
    assert _same(O1.cpu(), O2.cpu()) and _same(L1.cpu(), L2.cpu())


def test_forced_matrix_form_that_cannot_run_fails_before_the_cache_is_touched():
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    pool0 = _random_bytes((7, 1, 16, 576), dtype, g)
    table = torch.tensor([[0, 1, 2, 3], [4, 5, 6, 0], [1, 2, 3, 4]], dtype=torch.int32).to(DEV)
    pool, lens = pool0.to(DEV), torch.tensor([0, 15, 40], dtype=torch.int32).to(DEV)
    Q, new = torch.randn(B, H, 1, 576, generator=g).to(dtype).to(DEV), torch.randn(B, 1, 1, 576, generator=g).to(dtype).to(DEV)
    cos, sin = (t.to(DEV) for t in _tables(64, dtype, g))
    with pytest.raises(TypeError, match="page_size % 64"):
        fa.flash_attention_mla_decode_forward(Q, pool, lens, DEV, variant="mla16", block_table=table, kv_new=new, rotary_cos=cos,
                                              rotary_sin=sin)
    torch.cuda.synchronize()
    assert _same(pool.cpu(), pool0) and lens.cpu().tolist() == [0, 15, 40]
    # the same call without the forced form appends and attends
    O, L = fa.flash_attention_mla_decode_forward(Q, pool, lens, DEV, block_table=table, kv_new=new, rotary_cos=cos, rotary_sin=sin)
    torch.cuda.synchronize()
    assert not _same(pool.cpu(), pool0) and O.shape == (B, H, 1, 512)
