"""Packed MLA decode with fp8 queries (flash_attention_mla_varlen_decode_q8_forward) on the GPU: every packed row against plain float64
attention on q_descale * Q8 and kv_descale * KV8, rows no sequence owns untouched, every sequence bit for bit against the fixed q8 call on
that sequence alone, paged against contiguous and stale rows bit for bit.  The bars are tests/test_decode_mla_q8_gpu.py's: L from the
inputs; O of "mla8" twice the distance between the stated arithmetic restated in float64 (P8 = e4m3(256 p)) and the plain reference over
this file's cases (6.797e-2, computed here on the CPU: DESIGN.md has why) plus half an ulp of out_dtype; O of "generic" the 16-bit bar."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from test_decode_gpu import O_TOL
from test_decode_mla_q8_gpu import BF16, CAP, DEV, E4, F16, MASKS, SCALE, ids

pytestmark = pytest.mark.gpu
SEQS = [(0, 64), (1, 1), (1, 200), (2, 63), (3, 65), (5, 64), (3, 2), (4, 130)]  # (n_q, N_k)
CU, LENS = [0, 0, 1, 2, 4, 7, 12, 15, 19], [nk for _, nk in SEQS]
HEADS = [16, 72, 128]  # g = 16: four positions a tile; 72: a tile straddles positions unevenly; 128: two tiles a token
i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def case(H):
    """inputs from one seeded normal, quantised with a scalar descale"""
    g = torch.Generator().manual_seed(300 + H)
    q, kv = torch.randn(CU[-1], H, 576, generator=g), torch.randn(len(SEQS), 1, CAP, 576, generator=g)
    qd, kd = q.abs().max() / 448, kv.abs().max() / 448
    return (q / qd).to(E4), (kv / kd).to(E4), qd, kd


@functools.lru_cache(maxsize=None)
def reference(H, max_q, causal, window):
    """per packed row: plain float64 O, L (log2 domain); the stated arithmetic restated in float64; max sum |q8||k8|; the rows owned"""
    Q8, KV8, qd, kd = case(H)
    O, R = torch.zeros(CU[-1], H, 512, dtype=torch.float64), torch.zeros(CU[-1], H, 512, dtype=torch.float64)
    L, own, dots = torch.full((H, CU[-1]), math.inf, dtype=torch.float64), torch.zeros(CU[-1], dtype=torch.bool), 0.0
    for b, (n, nk) in enumerate(SEQS):
        n, s = min(n, max_q), CU[b]
        own[s:s + n] = True
        q8, k8 = Q8[s:s + n].double().transpose(0, 1), KV8[b, 0, :nk].double()  # (H, n, 576), (nk, 576)
        i, j = torch.arange(n)[:, None] + nk - n, torch.arange(nk)[None, :]
        vis = (j <= i + (0 if causal else window[1] if window else nk)) & (j >= i - (window[0] if window else nk))  # bottom-right band
        rows = vis.any(-1)
        if not rows.any():
            continue
        dots = max(dots, (q8.abs() @ k8.abs().T).max().item())
        S = ((qd.double() * q8) @ (kd.double() * k8).T * float(torch.tensor(SCALE, dtype=torch.float32)) * math.log2(math.e)).masked_fill(~vis, -math.inf)
        p = torch.exp2(S[:, rows] - S[:, rows].max(-1, keepdim=True).values)
        l, at = p.sum(-1, keepdim=True), torch.arange(s, s + n)[rows]
        O[at] = ((p / l) @ (kd.double() * k8[:, :512])).transpose(0, 1)
        R[at] = (kd.double() / 256 * ((256 * p).to(E4).double() @ k8[:, :512]) / l).transpose(0, 1)
        L[:, at] = S[:, rows].max(-1).values + torch.log2(l[..., 0])
    return O, L, R, dots, own


@functools.lru_cache(maxsize=None)
def allowance():
    """twice the restatement's largest distance from the plain reference over this file's cases"""
    worst = max((R - O).abs().max().item() for O, _, R, _, _ in (reference(H, q, *m) for H in HEADS for q in (3, 8) for m in MASKS))
    print(f"restatement against the plain reference: {worst:.3e}, allowance {2 * worst:.3e} + one rounding")
    return 2 * worst


def call(H, max_q=8, KV=None, **kw):
    Q8, KV8, qd, kd = case(H)
    return fa.flash_attention_mla_varlen_decode_q8_forward(Q8.to(DEV), (KV8 if KV is None else KV).to(DEV), i32(CU), max_q, i32(LENS), DEV,
                                                           q_descale=qd.to(DEV), kv_descale=kd.to(DEV), scale=SCALE, **kw)


@pytest.mark.parametrize("out_dtype", [F16, BF16], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "mla8", "generic"])
@pytest.mark.parametrize("max_q", [3, 5, 8])  # 3: below the counts 5 and 4; 8 declares tiles that hold no rows and moves the grid's rotation
@pytest.mark.parametrize("H", HEADS)
def test_forward_against_float64(H, max_q, variant, out_dtype):
    """through the library call itself, O and L pre-filled with 7: the rows no sequence owns (max_q = 3 alone has some) must keep it"""
    Q8, KV8, qd, kd = case(H)
    ws = torch.empty(_lib.kvcache_varlen_workspace_bytes(CU[-1], H, 512, 3) // 4, device=DEV)
    for causal, window in MASKS:
        O_ref, L_ref, _, dots, own = reference(H, max_q, causal, window)
        l_bar = 576 * 2.0 ** -24 * SCALE * qd.item() * kd.item() * dots + 2.0 ** -20
        half_ulp = 2.0 ** (math.floor(math.log2(O_ref.abs().max().item())) - (10 if out_dtype == F16 else 7) - 1)
        o_bar = O_TOL[out_dtype] if variant == "generic" else allowance() + half_ulp
        empty = torch.isinf(L_ref[:, own])
        for n in (1, 3):
            O, L = torch.full((CU[-1], H, 512), 7.0, dtype=out_dtype, device=DEV), torch.full((H, CU[-1]), 7.0, device=DEV)
            _lib.fa2_fwd_kvcache_mla_varlen_q8(Q8.to(DEV), KV8.to(DEV), O, L, i32(CU), max_q, i32(LENS), fa.convert_triton_dtype(out_dtype),
                                               _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E4M3, 512, q_descale=qd.to(DEV).expand(len(SEQS), 1),
                                               kv_descale=kd.to(DEV).expand(len(SEQS), 1), causal=causal, scale=SCALE, window=window,
                                               num_splits=n, workspace=ws, variant=_lib.KVCACHE_MLA_Q8_VARIANTS[variant])
            O, L = O.double().cpu(), L.double().cpu()
            assert (O[~own] == 7).all() and (L[:, ~own] == 7).all() and not torch.isnan(O).any() and not torch.isnan(L).any()
            O, L = O[own], L[:, own]
            assert torch.equal(torch.isinf(L), empty) and (L[empty] > 0).all() and (O.transpose(0, 1)[empty] == 0).all()
            l_err, o_err = (L[~empty] - L_ref[:, own][~empty]).abs().max().item(), (O - O_ref[own]).abs().max().item()
            print(f"{H} max_q={max_q} {variant} {out_dtype} {causal} {window} n={n}: L {l_err:.3e} (bar {l_bar:.3e}) O {o_err:.3e} (bar {o_bar:.3e})")
            assert l_err <= l_bar and o_err <= o_bar, (causal, window, n)


@pytest.mark.parametrize("variant", ["mla8", "generic"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("H", HEADS)
def test_each_sequence_equals_the_fixed_call_bit_for_bit(H, n, variant):
    Q8, KV8, qd, kd = case(H)
    for causal, window in MASKS:
        kw = dict(causal=causal, window=window, num_splits=n, variant=variant, out_dtype=F16)
        packed = [call(H, max_q, **kw) for max_q in (5, 8)]
        for b, (nq, nk) in enumerate(SEQS):
            s = CU[b]
            if nq == 0:
                continue
            Of, Lf = fa.flash_attention_mla_decode_q8_forward(Q8[s:s + nq].transpose(0, 1)[None].contiguous().to(DEV), KV8[b:b + 1].to(DEV), i32([nk]),
                                                              DEV, q_descale=qd.to(DEV), kv_descale=kd.to(DEV), scale=SCALE, **kw)
            for O, L in packed:
                assert O.dtype == F16 and L.dtype == torch.float32 and O.shape == (CU[-1], H, 512) and L.shape == (H, CU[-1])
                assert torch.equal(O[s:s + nq].transpose(0, 1).view(torch.int16), Of[0].view(torch.int16)) and torch.equal(L[:, s:s + nq], Lf[0]), (b, causal, window)


@pytest.mark.parametrize("variant", ["mla8", "generic"])
@pytest.mark.parametrize("page", [64, 128])
def test_paged_and_stale_rows_bit_for_bit(page, variant):
    KV8, kw, slots = case(72)[1].clone(), dict(causal=True, num_splits=3, variant=variant), len(SEQS) * CAP // page
    KV8[5, :, :page] = KV8[4, :, :page]  # sequences 4 and 5 share their first page
    O, L = call(72, KV=KV8, **kw)
    pages, table = KV8.view(torch.uint8).view(slots, page, 576), torch.empty(slots, dtype=torch.int32)
    table[torch.randperm(slots, generator=torch.Generator().manual_seed(page))] = torch.arange(slots, dtype=torch.int32)
    pool = torch.empty_like(pages)
    pool[table.long()] = pages  # page i of the cache sits at pool slot table[i]
    table = table.view(len(SEQS), -1).clone()
    table[5, 0] = table[4, 0]
    Op, Lp = call(72, KV=pool.view(E4).view(-1, 1, page, 576), block_table=table.to(DEV), **kw)
    assert torch.equal(Op.view(torch.int16), O.view(torch.int16)) and torch.equal(Lp, L)
    for byte in (0x7F, 0xFF):  # the NaN bytes of e4m3fn behind cache_seqlens
        stale = KV8.view(torch.uint8).clone()
        for b, nk in enumerate(LENS):
            stale[b, :, nk:] = byte
        Os, Ls = call(72, KV=stale.view(E4), **kw)
        assert torch.equal(Os.view(torch.int16), O.view(torch.int16)) and torch.equal(Ls, L)
