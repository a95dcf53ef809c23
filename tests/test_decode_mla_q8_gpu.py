"""MLA decode with fp8 queries over the fp8 latent cache (flash_attention_mla_decode_q8_forward) on the GPU: L and O against plain
attention in float64 on q_descale * Q8 and kv_descale * KV8, the exact cases, paged against contiguous and stale rows, bit for bit.

L: nothing but fp32 accumulation separates it from the reference: the bar is 576 * 2^-24 * scale * q_descale * kv_descale * max sum |q8||k8|
+ 2^-20, from the inputs.  O of "mla8": twice the distance between the stated arithmetic restated in float64 (P8 = e4m3(256 p)) and the
plain reference over this file's cases, plus one rounding of out_dtype; the restatement's distance computed here is 2.735e-2 at most
(|O| reaches 3.5; under its worst case 2^-4 * kv_descale * max |v8| = 0.31), so the allowance is 5.470e-2 + half an ulp of out_dtype at
max |O| (5.567e-2 for float16, 6.251e-2 for bfloat16; the kernel measured 2.74e-2 on an MI355X).  "generic" keeps P in fp32 and takes
the 16-bit bar of tests/test_decode_gpu.py."""
import functools
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from test_decode_gpu import O_TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E4, F16, BF16 = torch.float8_e4m3fn, torch.float16, torch.bfloat16
CAP, LENS, SCALE = 256, [0, 1, 63, 64, 65, 200], 576 ** -0.5
MASKS = ((False, None), (True, None), (False, (70, 0)))
ids = lambda x: str(x).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def case(H, N_q):
    """inputs from one seeded normal, quantised with a scalar descale, and the float64 results under every mask: plain and restated"""
    g = torch.Generator().manual_seed(100 * H + N_q)
    q, kv = torch.randn(len(LENS), H, N_q, 576, generator=g), torch.randn(len(LENS), 1, CAP, 576, generator=g)
    qd, kd = q.abs().max() / 448, kv.abs().max() / 448
    Q8, KV8 = (q / qd).to(E4), (kv / kd).to(E4)
    return Q8, KV8, qd, kd, {m: reference(Q8, KV8, qd, kd, *m) for m in MASKS}


def reference(Q8, KV8, qd, kd, causal, window):
    """plain attention in float64 -> O, L (log2 domain), the stated arithmetic restated in float64 -> O, and max sum |q8||k8|"""
    B, H, N_q, _ = Q8.shape
    O, R, L = torch.zeros(B, H, N_q, 512, dtype=torch.float64), torch.zeros(B, H, N_q, 512, dtype=torch.float64), torch.full((B, H, N_q), math.inf, dtype=torch.float64)
    dots = 0.0
    for b, nk in enumerate(LENS):
        q8, k8 = Q8[b].double(), KV8[b, 0, :nk].double()
        i, j = torch.arange(N_q)[:, None] + nk - N_q, torch.arange(nk)[None, :]
        vis = (j <= i + (0 if causal else window[1] if window else nk)) & (j >= i - (window[0] if window else nk))  # bottom-right band
        rows = vis.any(-1)
        if not rows.any():
            continue
        dots = max(dots, (q8.abs() @ k8.abs().T).max().item())
        S = ((qd.double() * q8) @ (kd.double() * k8).T * float(torch.tensor(SCALE, dtype=torch.float32)) * math.log2(math.e)).masked_fill(~vis, -math.inf)
        p = torch.exp2(S[:, rows] - S[:, rows].max(-1, keepdim=True).values)
        l = p.sum(-1, keepdim=True)
        O[b][:, rows] = (p / l) @ (kd.double() * k8[:, :512])
        R[b][:, rows] = kd.double() / 256 * ((256 * p).to(E4).double() @ k8[:, :512]) / l
        L[b][:, rows] = S[:, rows].max(-1).values + torch.log2(l[..., 0])
    return O, L, R, dots


@functools.lru_cache(maxsize=None)
def allowance():
    """twice the restatement's largest distance from the plain reference over this file's cases (and that distance under its worst case)"""
    worst = 0.0
    for H, N_q in SHAPES:
        Q8, KV8, qd, kd, refs = case(H, N_q)
        dist = max((R - O).abs().max().item() for O, _, R, _ in refs.values())
        assert dist <= 2.0 ** -4 * kd.item() * KV8.float().abs().max().item()
        worst = max(worst, dist)
    print(f"restatement against the plain reference: {worst:.3e}, allowance {2 * worst:.3e} + one rounding")
    return 2 * worst


SHAPES = [(16, 1), (72, 2), (128, 2)]


def call(Q8, KV8, qd, kd, lens=LENS, **kw):
    return fa.flash_attention_mla_decode_q8_forward(Q8.to(DEV), KV8.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), DEV,
                                                    q_descale=qd.to(DEV), kv_descale=kd.to(DEV), scale=SCALE, **kw)


@pytest.mark.parametrize("out_dtype", [F16, BF16], ids=ids)
@pytest.mark.parametrize("variant", ["auto", "mla8", "generic"])
@pytest.mark.parametrize("H,N_q", SHAPES)
def test_forward_against_float64(H, N_q, variant, out_dtype):
    Q8, KV8, qd, kd, refs = case(H, N_q)
    for (causal, window), (O_ref, L_ref, _, dots) in refs.items():
        l_bar = 576 * 2.0 ** -24 * SCALE * qd.item() * kd.item() * dots + 2.0 ** -20
        half_ulp = 2.0 ** (math.floor(math.log2(O_ref.abs().max().item())) - (10 if out_dtype == F16 else 7) - 1)
        o_bar = O_TOL[out_dtype] if variant == "generic" else allowance() + half_ulp
        for n in (1, 3):
            O, L = call(Q8, KV8, qd, kd, causal=causal, window=window, num_splits=n, variant=variant, out_dtype=out_dtype)
            assert O.dtype == out_dtype and L.dtype == torch.float32 and O.shape == (len(LENS), H, N_q, 512)
            O, L, empty = O.double().cpu(), L.double().cpu(), torch.isinf(L_ref)
            assert not torch.isnan(O).any() and not torch.isnan(L).any()          # every row is written
            assert torch.equal(torch.isinf(L), empty) and (L[empty] > 0).all() and (O[empty] == 0).all()
            l_err, o_err = (L[~empty] - L_ref[~empty]).abs().max().item(), (O - O_ref).abs().max().item()
            print(f"{H} {N_q} {variant} {out_dtype} causal={causal} window={window} n={n}: L {l_err:.3e} (bar {l_bar:.3e}) O {o_err:.3e} (bar {o_bar:.3e})")
            assert l_err <= l_bar and o_err <= o_bar, (causal, window, n)


@pytest.mark.parametrize("out_dtype", [F16, BF16], ids=ids)
@pytest.mark.parametrize("variant", ["mla8", "generic"])
@pytest.mark.parametrize("n", [1, 3])
def test_one_key_is_the_row_itself(n, variant, out_dtype):
    """N_k = 1: P is 1, 256 is representable, and O is kv_descale * v8 rounded once to out_dtype, bit for bit"""
    Q8, KV8, qd, kd, _ = case(72, 2)
    O, L = call(Q8, KV8, qd, kd, num_splits=n, variant=variant, out_dtype=out_dtype)
    want = (KV8[1, 0, 0, :512].float() * kd).to(out_dtype)
    assert torch.equal(O[1].cpu().view(torch.int16), want.expand(72, 2, 512).contiguous().view(torch.int16))
    assert (O[0] == 0).all() and (L[0] == math.inf).all()


@pytest.mark.parametrize("variant", ["mla8", "generic"])
@pytest.mark.parametrize("page", [64, 128])
def test_paged_and_stale_rows_bit_for_bit(page, variant):
    Q8, KV8, qd, kd, _ = case(72, 2)
    KV8 = KV8.clone()
    KV8[5, :, :page] = KV8[4, :, :page]  # sequences 4 and 5 share their first page
    kw = dict(causal=True, num_splits=3, variant=variant)
    O, L = call(Q8, KV8, qd, kd, **kw)
    per = CAP // page
    pages = KV8.view(torch.uint8).view(len(LENS) * per, page, 576)
    order = torch.randperm(len(LENS) * per, generator=torch.Generator().manual_seed(page))
    table = torch.empty(len(LENS) * per, dtype=torch.int32)
    table[order] = torch.arange(len(LENS) * per, dtype=torch.int32)  # page i of the cache sits at pool slot table[i]
    pool = torch.empty_like(pages)
    pool[table.long()] = pages
    table = table.view(len(LENS), per).clone()
    table[5, 0] = table[4, 0]
    Op, Lp = call(Q8, pool.view(E4).view(-1, 1, page, 576), qd, kd, block_table=table.to(DEV), **kw)
    assert torch.equal(Op.view(torch.int16), O.view(torch.int16)) and torch.equal(Lp, L)
    for byte in (0x7F, 0xFF):  # the NaN bytes of e4m3fn behind cache_seqlens
        stale = KV8.view(torch.uint8).clone()
        for b, nk in enumerate(LENS):
            stale[b, :, nk:] = byte
        Os, Ls = call(Q8, stale.view(E4), qd, kd, **kw)
        assert torch.equal(Os.view(torch.int16), O.view(torch.int16)) and torch.equal(Ls, L)
