"""mla_kvcache_append / _varlen with kv_format="fp8_ds" (fa2_kvcache_mla_append_ds, fa2_decode_append_q.hip) on the GPU: the 656 bytes
a token gets are quantize_mla_cache_ds (torch, on the CPU) of the row the 16-bit latent append stores, bit for bit, and no other byte of
a cache of random bytes changes."""
import pytest
import torch

import flash_attention_dlrs_amd as fa
from mla_append_restatement import expected_mla_append, expected_mla_append_packed
from test_decode_mla_append_gpu import B, DEV, LENS, LENS_CLAMPS, S_K, TABLE, _dev, _random_bytes, _tables  # the geometry of the 16-bit append's tests

pytestmark = pytest.mark.gpu


def _table(page, nb_seq, g):
    """(table, num_blocks): the 16-bit tests' table, else a shuffled one whose last entry is out of range (clamped to a page of its own)."""
    if page == 64 and nb_seq == B:
        return torch.tensor(TABLE, dtype=torch.int32), 7
    mb = S_K // page
    t = torch.randperm(nb_seq * mb, generator=g).to(torch.int32).view(nb_seq, mb)
    t[-1, -1] = 1 << 20
    return t, nb_seq * mb + 1


def _inputs(dtype, H_kv, lead, g):
    """c (*lead, 512), pe (*lead, 64), lead = (B, H_kv, N_new) or packed (total_new, H_kv), with the tile logic observable: tile t
    scaled by 2^(3 t), so a wrong tile-to-scale map fails; in the first token of entry 0 tile 1 is all zero (the 1e-4 floor), of entry
    1 tile 2's maximum is negative and in its first column, of entry 2 it is in the tile's last column."""
    c = torch.randn(*lead, 512, generator=g) * (8.0 ** torch.arange(4)).repeat_interleave(128)
    rows = c[:, :, 0] if len(lead) == 3 else c
    rows[0, :, 128:256] = 0.0
    rows[1, :, 256] = -5000.0
    rows[2, :, 383] = 5000.0
    return c.to(dtype), torch.randn(*lead, 64, generator=g).to(dtype)


def _quantised(KV8_0, KV16_0, want16):
    """The byte cache after the append: KV8_0 with quantize_mla_cache_ds of every row the 16-bit append wrote."""
    wrote = (want16.view(torch.int16) != KV16_0.view(torch.int16)).any(-1)
    want = KV8_0.clone()
    want[wrote] = fa.quantize_mla_cache_ds(want16[wrote])
    return want, int(wrote.sum())


class Problem:
    def __init__(self, dtype, H_kv, n_new, page, lens, rd, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.table, nb = _table(page, B, g) if page else (None, B)
        shape = (nb, H_kv, page or S_K)
        self.KV8_0, self.KV16_0 = _random_bytes(shape + (656,), torch.uint8, g), _random_bytes(shape + (576,), dtype, g)
        self.c, self.pe = _inputs(dtype, H_kv, (B, H_kv, n_new), g)
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.cos, self.sin = _tables(rd, dtype, g) if rd else (None, None)

    def expected(self, interleaved):
        want16, _, want_len = expected_mla_append(self.KV16_0, self.c, self.pe, self.lens, 512, self.table, None, self.cos, self.sin, interleaved)
        return _quantised(self.KV8_0, self.KV16_0, want16) + (want_len,)

    def run(self, kv_new, interleaved):
        KV, lens = self.KV8_0.to(DEV), self.lens.to(DEV)
        got = fa.mla_kvcache_append(KV, kv_new, lens, block_table=_dev(self.table), rotary_cos=_dev(self.cos), rotary_sin=_dev(self.sin),
                                    rotary_interleaved=interleaved, kv_format="fp8_ds")
        torch.cuda.synchronize()
        assert torch.equal(lens.cpu(), self.lens)
        return KV.cpu(), got.cpu()


@pytest.mark.parametrize("dtype,H_kv,n_new,page,lens,rd,interleaved,pair", [
    (torch.bfloat16, 1, 1, 0, LENS, 64, False, True),
    (torch.bfloat16, 2, 3, 64, LENS, 64, True, True),
    (torch.float16, 2, 3, 16, LENS, 32, False, False),       # a pass-through tail behind the rotary range; one (..., 576) tensor
    (torch.float16, 1, 3, 1, LENS_CLAMPS, 32, True, True),
    (torch.bfloat16, 2, 3, 0, LENS_CLAMPS, 0, False, False),  # no rotary at all
    (torch.float16, 1, 1, 16, LENS, 64, False, True),
])
def test_written_bytes_are_quantize_mla_cache_ds_of_the_16_bit_row(dtype, H_kv, n_new, page, lens, rd, interleaved, pair):
    p = Problem(dtype, H_kv, n_new, page, lens, rd, seed=1)
    want, _, want_len = p.expected(interleaved)
    kv_new = (p.c.to(DEV), p.pe.to(DEV)) if pair else torch.cat([p.c, p.pe], dim=-1).to(DEV)
    got, got_len = p.run(kv_new, interleaved)
    assert torch.equal(got_len, want_len), (got_len, want_len)
    assert torch.equal(got, want), f"{(got != want).sum().item()} bytes differ"


@pytest.mark.parametrize("interleaved", [False, True])
def test_element_form_on_a_misaligned_strided_view_gives_the_vector_forms_bytes(interleaved):
    p = Problem(torch.bfloat16, 2, 3, 16, LENS, 32, seed=2)
    want, _, _ = p.expected(interleaved)
    vec, _ = p.run((p.c.to(DEV), p.pe.to(DEV)), interleaved)
    assert torch.equal(vec, want)
    odd = torch.zeros(p.c.numel() + 1, dtype=p.c.dtype, device=DEV)[1:].view(p.c.shape)
    odd.copy_(p.c)                                                                         # misaligned by one element
    wide = torch.zeros(*p.pe.shape[:3], 128, dtype=p.pe.dtype, device=DEV)[..., ::2]
    wide.copy_(p.pe)                                                                       # a column stride of 2
    assert odd.data_ptr() % 16 == 2 and wide.stride(3) == 2
    assert torch.equal(p.run((odd, wide), interleaved)[0], vec)


CU, MAX_NEW, LENS4 = [0, 3, 3, 4, 9], 4, [63, 5, 190, 0]   # an empty sequence and a span of 5 cut to 4


@pytest.mark.parametrize("page,rd,interleaved", [(0, 64, False), (16, 32, True)])
def test_packed_form(page, rd, interleaved):
    dtype, H_kv, nb_seq = torch.float16, 2, 4
    g = torch.Generator().manual_seed(3)
    table, nb = _table(page, nb_seq, g) if page else (None, nb_seq)
    KV8_0, KV16_0 = _random_bytes((nb, H_kv, page or S_K, 656), torch.uint8, g), _random_bytes((nb, H_kv, page or S_K, 576), dtype, g)
    c, pe = _inputs(dtype, H_kv, (9, H_kv), g)
    cu, lens = torch.tensor(CU, dtype=torch.int32), torch.tensor(LENS4, dtype=torch.int32)
    cos, sin = _tables(rd, dtype, g) if rd else (None, None)
    want16, want_len = expected_mla_append_packed(KV16_0, c, pe, cu, MAX_NEW, lens, 512, table, None, cos, sin, interleaved)
    want, rows = _quantised(KV8_0, KV16_0, want16)
    assert want_len.tolist() == [66, 5, 191, 4] and rows == 8 * H_kv
    kw = dict(block_table=_dev(table), rotary_cos=_dev(cos), rotary_sin=_dev(sin), rotary_interleaved=interleaved, kv_format="fp8_ds")
    KV, lens_d = KV8_0.to(DEV), lens.to(DEV)
    got_len = fa.mla_kvcache_append_varlen(KV, (c.to(DEV), pe.to(DEV)), cu.to(DEV), MAX_NEW, lens_d, **kw)
    torch.cuda.synchronize()
    assert torch.equal(lens_d.cpu(), lens) and torch.equal(got_len.cpu(), want_len)
    assert torch.equal(KV.cpu(), want), f"{(KV.cpu() != want).sum().item()} bytes differ"
    KV2 = KV8_0.to(DEV)                                     # ... and the fixed call, sequence by sequence
    for b in range(nb_seq):
        s, n = CU[b], min(CU[b + 1] - CU[b], MAX_NEW)
        if n:
            fixed = lambda x: x[s:s + n].transpose(0, 1).unsqueeze(0).to(DEV)
            kw["block_table"] = None if table is None else table[b:b + 1].to(DEV)
            new = fa.mla_kvcache_append(KV2 if page else KV2[b:b + 1], (fixed(c), fixed(pe)), lens_d[b:b + 1], **kw)
            assert new.cpu().tolist() == [want_len[b].item()]
    assert torch.equal(KV2.cpu(), KV.cpu())


def test_sparse_decode_over_the_appended_cache_equals_the_torch_built_one():
    g = torch.Generator().manual_seed(4)
    n, H = 128, 16
    kv16 = (torch.randn(2, 1, n, 576, generator=g) * 0.5).to(torch.bfloat16)
    built = fa.quantize_mla_cache_ds(kv16).to(DEV)
    appended = torch.zeros_like(built)
    zero = torch.zeros(2, dtype=torch.int32, device=DEV)
    lens = fa.mla_kvcache_append(appended, kv16.to(DEV), zero, kv_format="fp8_ds")
    assert lens.tolist() == [n, n] and torch.equal(appended, built)
    Q = torch.randn(2, H, 1, 576, generator=g).to(torch.bfloat16).to(DEV)
    idx = torch.randint(0, n, (2, 1, 64), generator=g).to(torch.int32).to(DEV)
    outs = [fa.flash_attention_mla_sparse_decode_forward(Q, kv, idx, lens, DEV, scale=576 ** -0.5, kv_format="fp8_ds") for kv in (appended, built)]
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
