"""The indexer's front end on the GPU (fa2_indexer_prep.hip): mla_indexer_prepare_queries / _varlen and the rotary / hadamard keywords
of mla_indexer_append / _varlen against their statement in torch on the CPU -- apply_rotary, hadamard_rotate, quantize_index_keys --
bit for bit, and against rotary and the Hadamard matrix in fp64 within a derived bound."""
import itertools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from test_decode_mla_append_gpu import B, DEV, LENS, LENS_CLAMPS, S_K, _dev, _random_bytes as _random
from test_decode_mla_append_ds_gpu import _table
from test_mla_indexer_append_gpu import _bits, _expected
from test_mla_indexer_prepare_host import H128

pytestmark = pytest.mark.gpu

E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
S_ROT, N_Q, Q_LENS = 32, 3, [1, 40, 7]  # query positions -2 .. 0 (clamped to 0), 37 .. 39 (clamped to 31) and 4 .. 6
# n leading columns of value v: the transformed row's maximum, in column 0, rounds to 1.75 * 2^k = finfo(fp8).max * 2^j in the dtype
EXACT = {torch.float16: (93, 1.703125), torch.bfloat16: (11, 1.796875)}
ROTARY = [(0, False), (64, False), (64, True), (128, False), (128, True)]


def _rows(shape, dtype, g):
    """Rows with magnitudes spread over 2^-6 .. 2^6.  Row 0 is zero; row 1 has a transformed maximum of exactly 1.75 * 2^k (EXACT) and
    row 2 an untransformed one: the m == 0.5 branch of the scale, with and without the Hadamard step (and no rotation)."""
    x = (torch.randn(*shape, 128, generator=g) * 2.0 ** torch.randint(-6, 7, (*shape, 1), generator=g)).to(dtype)
    flat = x.view(-1, 128)
    flat[:3] = 0
    flat[1, :EXACT[dtype][0]] = EXACT[dtype][1]
    flat[2] = (torch.randn(128, generator=g) * 1e-2).to(dtype)
    flat[2, 127] = -14.0
    return x


def _strided(t):
    """t on the device with t's own strides (Tensor.to compacts a view that is not dense)."""
    return None if t is None else torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV).copy_(t)


def _tables(rd, dtype, g, aligned=True, s_rot=S_ROT):
    """cos, sin (s_rot, rd / 2) of random angles; aligned=False: rows rd / 2 + 4 elements apart, off the kernel's 16-byte table loads."""
    if not rd:
        return None, None
    ang = torch.rand(s_rot, rd // 2, generator=g) * 6.28
    hold = [torch.zeros(s_rot, rd // 2 + (0 if aligned else 4), dtype=dtype) for _ in range(2)]
    hold[0][:, :rd // 2], hold[1][:, :rd // 2] = ang.cos().to(dtype), ang.sin().to(dtype)
    return hold[0][:, :rd // 2], hold[1][:, :rd // 2]


def _restate(x, cos, sin, pos, interleaved, hadamard):
    """Steps 1 and 2 of the statement; pos broadcasts to x's rows."""
    r = x if cos is None else fa.apply_rotary(x, cos, sin, pos, interleaved)
    return fa.hadamard_rotate(r) if hadamard else r


def _restate_q(q, w, pos, out, weight_scale, cos, sin, interleaved, hadamard):
    h = _restate(q, cos, sin, pos, interleaved, hadamard)
    if out is None:
        return h, w * weight_scale, h, None
    q8, scale = fa.quantize_index_keys(h, out)
    return q8, (w * weight_scale) * scale, h, scale


@pytest.mark.parametrize("hadamard", [True, False])
@pytest.mark.parametrize("rd,interleaved", ROTARY)
@pytest.mark.parametrize("dtype,out", list(itertools.product((torch.float16, torch.bfloat16), (E4, E5, None))))
def test_queries_are_the_statement_bit_for_bit(dtype, out, rd, interleaved, hadamard):
    g = torch.Generator().manual_seed(5)
    lens = torch.tensor(Q_LENS, dtype=torch.int32)
    pos = (lens[:, None] - N_Q + torch.arange(N_Q))[:, None, :]
    for H_I in (5, 64):  # 5: a partial tile of heads, and the element paths (rows and tables off their 16-byte alignment); 64: four tiles
        cos, sin = _tables(rd, dtype, g, aligned=H_I == 64)
        q = _rows((B, N_Q, H_I), dtype, g)
        if H_I == 5:  # rows 132 elements apart
            q = torch.cat((q, q.new_zeros(B, N_Q, H_I, 4)), -1)[..., :128]
        q = q.permute(0, 2, 1, 3)  # (B, H_I, N_q, 128), a strided view: flat row r of _rows is q[0, r, 0]
        w = torch.randn(B, N_Q, H_I, generator=g).permute(0, 2, 1)
        want_q, want_w, h, scale = _restate_q(q, w, pos, out, 0.125, cos, sin, interleaved, hadamard)
        if out is not None and not rd:
            m = torch.frexp(h[0, 1 if hadamard else 2, 0].float().abs().max() / torch.finfo(out).max)[0]
            assert m == 0.5 and scale[0, 0, 0] == 1  # the inputs do reach the exact branch, and the row of zeros
        got_q, got_w = fa.mla_indexer_prepare_queries(_strided(q), _strided(w), _dev(lens), dtype=out, weight_scale=0.125,
                                                      rotary_cos=_strided(cos), rotary_sin=_strided(sin), rotary_interleaved=interleaved,
                                                      hadamard=hadamard)
        assert got_q.is_contiguous() and got_w.is_contiguous() and got_q.dtype == want_q.dtype
        want_q = want_q.contiguous()
        assert torch.equal(_bits(got_q.cpu()), _bits(want_q)), f"H_I {H_I}: {(_bits(got_q.cpu()) != _bits(want_q)).sum().item()} differ"
        assert torch.equal(got_w.cpu(), want_w), H_I


@pytest.mark.parametrize("dtype,out", [(torch.float16, E4), (torch.bfloat16, E5), (torch.bfloat16, None)])
def test_queries_against_rotary_and_the_hadamard_matrix_in_fp64(dtype, out):
    """q_out * q_scale against ref = H rot(x) / sqrt(128) in fp64.  Four terms, none fitted: (1) the fp8 rounding, half a step of the
    element at its scale: 2^-4 |q| q_scale (e4m3, 3 mantissa bits) or 2^-3 (e5m2), at least half the smallest subnormal step (2^-10 or
    2^-17) times q_scale -- none for a 16-bit q_out; (2) 2^-9 ||x||_2: the rotation's result is rounded to the dtype, a relative 2^-9
    (bf16; f16 is finer) of each element, so an error vector of norm <= 2^-9 ||r||_2 = 2^-9 ||x||_2, which the orthonormal transform
    carries into any one column at full size at most; (3) 2^-9 |ref|: the 16-bit rounding of h; (4) 7 * 2^-24 ||x||_1 / sqrt(128): the
    fp32 stages (test_mla_indexer_prepare_host)."""
    g = torch.Generator().manual_seed(6)
    H_I, lens = 8, torch.tensor(Q_LENS, dtype=torch.int32)
    pos = (lens[:, None] - N_Q + torch.arange(N_Q))[:, None, :].clamp(0, S_ROT - 1).expand(B, H_I, N_Q)
    q = _rows((B, H_I, N_Q), dtype, g)
    ang = torch.rand(S_ROT, 32, generator=g) * 6.28
    cos, sin = ang.cos().to(dtype), ang.sin().to(dtype)
    got_q, got_w = fa.mla_indexer_prepare_queries(_dev(q), torch.ones(B, H_I, N_Q, device=DEV), _dev(lens), dtype=out, rotary_cos=_dev(cos),
                                                  rotary_sin=_dev(sin))
    x, c, s = q.double(), cos.double()[pos], sin.double()[pos]
    rot = torch.cat((x[..., :32] * c - x[..., 32:64] * s, x[..., 32:64] * c + x[..., :32] * s, x[..., 64:]), -1)
    ref = rot @ H128 / 128 ** 0.5
    scale = got_w.cpu().double()[..., None]  # weights of 1 and weight_scale = 1: weights_out IS q_scale
    val = got_q.cpu().double() * scale
    step = {E4: (2.0 ** -4, 2.0 ** -10), E5: (2.0 ** -3, 2.0 ** -17), None: (0.0, 0.0)}[out]
    bound = torch.maximum(step[0] * val.abs(), step[1] * scale) + 2.0 ** -9 * x.norm(dim=-1, keepdim=True) + 2.0 ** -9 * ref.abs() \
        + 7 * 2.0 ** -24 * x.abs().sum(-1, keepdim=True) / 128 ** 0.5
    err = (val - ref).abs()
    print(f"max err / bound = {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert (err <= bound).all()


CU_Q, MAX_Q, LENS4 = [0, 3, 3, 5, 9], 3, [1, 9, 40, 7]  # an empty sequence; a span of 4 cut to 3: packed row 8 belongs to nobody


@pytest.mark.parametrize("dtype,out,H_I", [(torch.bfloat16, E4, 5), (torch.float16, None, 64)])
def test_packed_queries_are_the_fixed_call_per_sequence(dtype, out, H_I):
    g = torch.Generator().manual_seed(7)
    cos, sin = (_dev(t) for t in _tables(64, dtype, g))
    q, w = _dev(_rows((9, H_I), dtype, g)), _dev(torch.randn(9, H_I, generator=g))
    lens = torch.tensor(LENS4, dtype=torch.int32, device=DEV)
    out_dtype = dtype if out is None else out
    q_out = torch.full((9 * H_I * 128 * (1 if out else 2),), 0x5A, dtype=torch.uint8, device=DEV).view(out_dtype).view(9, H_I, 128)  # canaries
    w_out = torch.full((9, H_I), 7.0, device=DEV)
    _lib.fa2_mla_indexer_prepare_q(q, w, q_out, w_out, lens, convert_triton_dtype(dtype), convert_triton_dtype(out_dtype), weight_scale=0.5,
                                   rotary_cos=cos, rotary_sin=sin, cu_q=torch.tensor(CU_Q, dtype=torch.int32, device=DEV), max_q=MAX_Q)
    assert (q_out[8].view(torch.uint8) == 0x5A).all() and (w_out[8] == 7.0).all()
    for b in range(4):
        n = min(CU_Q[b + 1] - CU_Q[b], MAX_Q)
        if n:
            rows = slice(CU_Q[b], CU_Q[b] + n)
            fq, fw = fa.mla_indexer_prepare_queries(q[rows].transpose(0, 1)[None], w[rows].T[None], lens[b:b + 1], dtype=out, weight_scale=0.5,
                                                    rotary_cos=cos, rotary_sin=sin)
            assert torch.equal(_bits(q_out[rows]), _bits(fq[0].transpose(0, 1))) and torch.equal(w_out[rows], fw[0].T), b
    via_wrapper = fa.mla_indexer_prepare_queries_varlen(q, w, torch.tensor(CU_Q, dtype=torch.int32, device=DEV), MAX_Q, lens, dtype=out,
                                                        weight_scale=0.5, rotary_cos=cos, rotary_sin=sin)
    assert torch.equal(_bits(via_wrapper[0][:8]), _bits(q_out[:8])) and torch.equal(via_wrapper[1][:8], w_out[:8])


def _transformed(per_seq, lens, cap, cos, sin, interleaved, hadamard):
    """What each sequence's rows become before they are stored: row t of sequence b at key index clamp(lens[b], 0, cap) + t."""
    out = []
    for b, rows in enumerate(per_seq):
        pos = min(max(int(lens[b]), 0), cap) + torch.arange(len(rows))
        out.append(_restate(rows, cos, sin, pos, interleaved, hadamard) if len(rows) else rows)
    return out


@pytest.mark.parametrize("dtype,k_dtype,page,lens,rd,interleaved,hadamard", [
    (torch.bfloat16, E4, 0, LENS, 64, False, True),
    (torch.float16, E5, 1, LENS, 64, True, True),
    (torch.bfloat16, None, 16, LENS_CLAMPS, 128, False, True),
    (torch.float16, E4, 48, LENS_CLAMPS, 64, False, False),
    (torch.bfloat16, E5, 16, LENS, 0, False, True),
])
def test_appended_keys_are_the_statement_bit_for_bit(dtype, k_dtype, page, lens, rd, interleaved, hadamard):
    """Contiguous and paged (pages of 1, 16 and 48 rows), sequence 2 overflowing its capacity; the cache and the scales start as random
    bytes, so every row and scale behind a length is a canary."""
    g = torch.Generator().manual_seed(8)
    table, nb = _table(page, B, g) if page else (None, B)
    K0 = _random((nb, page or S_K, 128), k_dtype or dtype, g)
    S0 = _random((nb, page or S_K), torch.float32, g) if k_dtype else None
    cos, sin = _tables(rd, dtype, g, s_rot=100)  # positions 0 .. 2 and 63 .. 65, and 190, 191 clamped to 99
    k_new = _rows((B, 3), dtype, g)
    lens = torch.tensor(lens, dtype=torch.int32)
    want_K, want_S, want_len = _expected(K0, S0, _transformed(list(k_new), lens, S_K, cos, sin, interleaved, hadamard), lens, table)
    K, S = _dev(K0), _dev(S0)
    got = fa.mla_indexer_append(K, _dev(k_new), _dev(lens), k_scale=S, block_table=_dev(table), rotary_cos=_dev(cos), rotary_sin=_dev(sin),
                                rotary_interleaved=interleaved, hadamard=hadamard)
    assert torch.equal(got.cpu(), want_len) and not torch.equal(_bits(want_K), _bits(K0))
    assert torch.equal(_bits(K.cpu()), _bits(want_K)), f"{(_bits(K.cpu()) != _bits(want_K)).sum().item()} elements differ"
    assert S0 is None or torch.equal(_bits(S.cpu()), _bits(want_S))


@pytest.mark.parametrize("k_dtype,page", [(E4, 16), (None, 0)])
def test_packed_append_and_the_default_keywords(k_dtype, page):
    g = torch.Generator().manual_seed(9)
    dtype, cu, lens = torch.bfloat16, torch.tensor(CU_Q, dtype=torch.int32), torch.tensor([63, 5, 190, 0], dtype=torch.int32)
    table, nb = _table(page, 4, g) if page else (None, 4)
    K0 = _random((nb, page or S_K, 128), k_dtype or dtype, g)
    S0 = _random((nb, page or S_K), torch.float32, g) if k_dtype else None
    cos, sin = _tables(64, dtype, g, s_rot=100)
    k_new = _rows((9,), dtype, g)
    per_seq = [k_new[CU_Q[b]:CU_Q[b] + min(CU_Q[b + 1] - CU_Q[b], MAX_Q)] for b in range(4)]
    want_K, want_S, want_len = _expected(K0, S0, _transformed(per_seq, lens, S_K, cos, sin, False, True), lens, table)
    K, S = _dev(K0), _dev(S0)
    got = fa.mla_indexer_append_varlen(K, _dev(k_new), _dev(cu), MAX_Q, _dev(lens), k_scale=S, block_table=_dev(table), rotary_cos=_dev(cos),
                                       rotary_sin=_dev(sin), hadamard=True)
    assert torch.equal(got.cpu(), want_len) and torch.equal(_bits(K.cpu()), _bits(want_K))
    assert S0 is None or torch.equal(_bits(S.cpu()), _bits(want_S))
    # the default keywords make the old call: the same bytes as the entry point without the keywords' arguments
    K1, S1, K2, S2 = _dev(K0), _dev(S0), _dev(K0), _dev(S0)
    fa.mla_indexer_append_varlen(K1, _dev(k_new), _dev(cu), MAX_Q, _dev(lens), k_scale=S1, block_table=_dev(table))
    out2 = torch.empty(4, dtype=torch.int32, device=DEV)
    _lib.fa2_mla_indexer_append(K2, S2, _dev(k_new), _dev(lens), out2, convert_triton_dtype(dtype), convert_triton_dtype(K0.dtype),
                                block_table=_dev(table), cu_new=_dev(cu), max_new=MAX_Q)
    assert torch.equal(_bits(K1), _bits(K2)) and (S0 is None or torch.equal(_bits(S1), _bits(S2))) and not torch.equal(_bits(K1), _bits(K))


def test_prepared_operands_give_the_indexer_the_torch_prepared_lists():
    g = torch.Generator().manual_seed(10)
    n, H_I, dtype = 160, 8, torch.bfloat16
    cos, sin = _tables(64, dtype, g, s_rot=200)
    k = (torch.randn(2, n, 128, generator=g) * 2.0 ** torch.randint(-4, 5, (2, n, 1), generator=g)).to(dtype)
    q, w = torch.randn(2, H_I, 2, 128, generator=g).to(dtype), torch.rand(2, H_I, 2, generator=g)
    lens = torch.tensor([n, n], dtype=torch.int32)
    k8, ks = (_dev(t) for t in fa.quantize_index_keys(_restate(k, cos, sin, torch.arange(n)[None], False, True), E4))
    q8, w8, _, _ = _restate_q(q, w, (n - 2 + torch.arange(2))[None, None], E4, 0.25, cos, sin, False, True)
    a8, a_s = torch.zeros_like(k8), torch.zeros_like(ks)
    got_len = fa.mla_indexer_append(a8, _dev(k), torch.zeros(2, dtype=torch.int32, device=DEV), k_scale=a_s, rotary_cos=_dev(cos),
                                    rotary_sin=_dev(sin), hadamard=True)
    p8, pw = fa.mla_indexer_prepare_queries(_dev(q), _dev(w), got_len, weight_scale=0.25, rotary_cos=_dev(cos), rotary_sin=_dev(sin))
    lists = [fa.flash_attention_mla_indexer_topk(qq, ww, kk, _dev(lens), DEV, topk=32, k_scale=ss)
             for qq, ww, kk, ss in ((p8, pw, a8, a_s), (_dev(q8), _dev(w8), k8, ks))]
    assert got_len.tolist() == [n, n] and torch.equal(*lists)
