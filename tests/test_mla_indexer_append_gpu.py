"""mla_indexer_append / _varlen (fa2_mla_indexer_append, fa2_decode_append_q.hip) on the GPU: the bytes and scales a key gets are
quantize_index_keys (torch, on the CPU) of its row, bit for bit -- or the row itself in a cache of its dtype -- and nothing else of a
cache of random bytes changes."""
import pytest
import torch

import flash_attention_dlrs_amd as fa
from test_decode_mla_append_gpu import B, DEV, LENS, LENS_CLAMPS, S_K, _dev, _random_bytes as _random  # the geometry of the latent append's tests
from test_decode_mla_append_ds_gpu import _table

pytestmark = pytest.mark.gpu

INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2


def _bits(t):
    return t.view(INT[t.element_size()])


def _keys(n, d, dtype, top, g):
    """(n, d) keys with magnitudes spread over 2^-8 .. 2^8; row 0 has amax exactly top / 4 (the scale's exponent steps there), row 1
    the next value of dtype above it, row 2 is zero."""
    k = (torch.randn(n, d, generator=g) * 2.0 ** torch.randint(-8, 9, (n, 1), generator=g)).to(dtype)
    k[:3] = (torch.randn(3, d, generator=g) * 1e-2).to(dtype)
    k[0, d - 1] = -top / 4
    k[1, 0] = top / 4
    _bits(k)[1, 0] += 1
    k[2] = 0
    assert k[1, 0].float() > top / 4 and k[0].float().abs().max() == top / 4
    return k


def _expected(K0, S0, per_seq, lens, table):
    """(cache, scales, new lengths) after sequence b appended the rows per_seq[b], on the CPU."""
    K, S = K0.clone(), None if S0 is None else S0.clone()
    P = K0.shape[1]
    cap = P if table is None else table.shape[1] * P
    out = []
    for b, rows in enumerate(per_seq):
        start = min(max(int(lens[b]), 0), cap)
        out.append(min(start + len(rows), cap))
        if len(rows) and S is not None:
            rows, sc = fa.quantize_index_keys(rows, K0.dtype)
        for t in range(min(len(rows), cap - start)):
            j = start + t
            blk, row = (b, j) if table is None else (min(max(int(table[b, j // P]), 0), K0.shape[0] - 1), j % P)
            _bits(K)[blk, row] = _bits(rows)[t]
            if S is not None:
                S[blk, row] = sc[t]
    return K, S, torch.tensor(out, dtype=torch.int32)


def _check(K0, S0, k_new, per_seq, lens, table, strided=False, **packed):
    want_K, want_S, want_len = _expected(K0, S0, per_seq, lens, table)
    K, lens_d, k_new = K0.to(DEV), lens.to(DEV), k_new.to(DEV)
    S = _dev(S0)
    if strided:  # a column stride of 2 in k_new and in the scales: the general form
        k_new = torch.zeros(*k_new.shape[:-1], 2 * k_new.shape[-1], dtype=k_new.dtype, device=DEV)[..., ::2].copy_(k_new)
        S = torch.zeros(*S.shape, 2, device=DEV)[..., 0].copy_(S)
    if packed:
        got = fa.mla_indexer_append_varlen(K, k_new, packed["cu"].to(DEV), packed["max_new"], lens_d, k_scale=S, block_table=_dev(table))
    else:
        got = fa.mla_indexer_append(K, k_new, lens_d, k_scale=S, block_table=_dev(table))
    torch.cuda.synchronize()
    assert torch.equal(lens_d.cpu(), lens) and torch.equal(got.cpu(), want_len), (got, want_len)
    assert not torch.equal(_bits(want_K), _bits(K0))
    assert torch.equal(_bits(K.cpu()), _bits(want_K)), f"{(_bits(K.cpu()) != _bits(want_K)).sum().item()} elements differ"
    if S0 is not None:
        assert torch.equal(_bits(S.cpu()), _bits(want_S)), f"{(_bits(S.cpu()) != _bits(want_S)).sum().item()} scales differ"
    return K, S


@pytest.mark.parametrize("dtype,k_dtype,d,n_new,page,lens,strided", [
    (torch.bfloat16, E4, 128, 1, 0, LENS, False),
    (torch.float16, E4, 128, 3, 64, LENS, False),
    (torch.bfloat16, E5, 128, 3, 16, LENS_CLAMPS, False),
    (torch.float16, E5, 128, 3, 0, LENS, True),           # d_I = 128 off the vector form
    (torch.bfloat16, E4, 96, 3, 16, LENS, False),         # the general form
    (torch.float16, E5, 96, 3, 0, LENS_CLAMPS, True),
])
def test_bytes_and_scales_are_quantize_index_keys_of_the_row(dtype, k_dtype, d, n_new, page, lens, strided):
    g = torch.Generator().manual_seed(1)
    table, nb = _table(page, B, g) if page else (None, B)
    K0, S0 = _random((nb, page or S_K, d), k_dtype, g), _random((nb, page or S_K), torch.float32, g)
    k_new = _keys(B * n_new, d, dtype, torch.finfo(k_dtype).max, g).view(B, n_new, d)
    _check(K0, S0, k_new, list(k_new), torch.tensor(lens, dtype=torch.int32), table, strided)


@pytest.mark.parametrize("dtype,d,page", [(torch.float16, 128, 16), (torch.float32, 96, 0)])
def test_same_dtype_cache_takes_a_copy_of_bits(dtype, d, page):
    g = torch.Generator().manual_seed(2)
    table, nb = _table(page, B, g) if page else (None, B)
    K0, k_new = _random((nb, page or S_K, d), dtype, g), _random((B, 3, d), dtype, g)   # any bit pattern, NaNs included
    _check(K0, None, k_new, list(k_new), torch.tensor(LENS, dtype=torch.int32), table)


CU, MAX_NEW, LENS4 = [0, 3, 3, 4, 9], 4, [63, 5, 190, 0]   # an empty sequence and a span of 5 cut to 4


@pytest.mark.parametrize("d,page", [(128, 16), (96, 0)])
def test_packed_form(d, page):
    g = torch.Generator().manual_seed(3)
    table, nb = _table(page, 4, g) if page else (None, 4)
    K0, S0 = _random((nb, page or S_K, d), E4, g), _random((nb, page or S_K), torch.float32, g)
    k_new = _keys(9, d, torch.bfloat16, 448.0, g)
    per_seq = [k_new[CU[b]:CU[b] + min(CU[b + 1] - CU[b], MAX_NEW)] for b in range(4)]
    _check(K0, S0, k_new, per_seq, torch.tensor(LENS4, dtype=torch.int32), table, cu=torch.tensor(CU, dtype=torch.int32), max_new=MAX_NEW)


def test_indexer_lists_over_the_appended_cache_are_the_torch_built_ones():
    g = torch.Generator().manual_seed(4)
    n, H_I, d = 160, 8, 128
    k = (torch.randn(2, n, d, generator=g) * 2.0 ** torch.randint(-4, 5, (2, n, 1), generator=g)).to(torch.bfloat16)
    k8, ks = (t.to(DEV) for t in fa.quantize_index_keys(k, E4))
    a8, a_s = torch.zeros_like(k8), torch.zeros_like(ks)
    lens = fa.mla_indexer_append(a8, k.to(DEV), torch.zeros(2, dtype=torch.int32, device=DEV), k_scale=a_s)
    assert lens.tolist() == [n, n] and torch.equal(_bits(a8), _bits(k8)) and torch.equal(a_s, ks)
    q = torch.randn(2, H_I, 2, d, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.rand(2, H_I, 2, generator=g).to(DEV)
    lists = [fa.flash_attention_mla_indexer_topk(q, w, kk, lens, DEV, topk=32, k_scale=ss) for kk, ss in ((a8, a_s), (k8, ks))]
    assert torch.equal(*lists)
