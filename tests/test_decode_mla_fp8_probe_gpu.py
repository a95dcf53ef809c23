"""MLA decode over an fp8 latent cache (fa2_fwd_kvcache_mla_fp8) through the exact-arithmetic probe of tests/mla_fp8_probe.py, by the
Python surface: the bars, the truth and the cases are tests/test_decode_mla_probe_gpu.py's (O within one output ulp of the fp64
truth, exact zeros, L within one ulp, exact empty rows), the cache is the same latent rows stored in e4m3fn / e5m2 under a descale
of 2 or of 0.25 -- exact in both formats.  tests/test_decode_mla_fp8_probe.py shows on the CPU that a descale left out or applied
twice, exchanged halves of a load or pairs of a word, a row fetched at the 16-bit stride and a tail taken from the 16-bit map's
offsets fail these bars on every configuration run here."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
import mla_fp8_probe as P
import mla_probe as M
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D
from test_decode_mla_probe_gpu import B, DEV, cache, case, ids, scatter

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2


@functools.lru_cache(maxsize=None)
def stored(descale, fmt):
    """the latent rows in fp8 under kv_descale = descale: built once, never modified"""
    KV8 = P.stored(cache(), descale, fmt)
    assert torch.equal(P.dequantised(KV8, descale), cache())
    return KV8


def run(dtype, variant, cfgs, KV8, descale, **kw):
    """the probe, scored and uniform, over `cfgs` on the fp8 latent cache KV8 (any form) -> [(case, probe, violations)]"""
    bad = []
    lens = torch.tensor(list(M.LENS), dtype=torch.int32, device=DEV)
    kv_descale = torch.full((B, 1), descale, dtype=torch.float32, device=DEV)
    for H, n_q, causal, window, n in cfgs:
        resolved = n or _lib.kvcache_mla_num_splits(B, H, 1, n_q, M.S_K, 576, 512, convert_triton_dtype(dtype))
        for uniform in (False, True):
            Q, O_ref, L_ref = case(H, n_q, causal, window, uniform)
            O, L = fa.flash_attention_mla_decode_forward(Q.to(dtype), KV8, lens, DEV, causal=causal, scale=D.SCALE, window=window,
                                                         num_splits=n, variant=variant, kv_descale=kv_descale, **kw)
            assert O.shape == (B, H, n_q, 512) and O.dtype == dtype and L.dtype == dtype
            v = M.violations(O, L, O_ref, L_ref, dtype, resolved > 1)
            if v:
                bad.append(((H, n_q, causal, window, n, resolved), "uniform" if uniform else "scored", v))
    return bad


FWD = [(fmt, dt, v) for fmt in (E4, E5) for dt in (F16, BF16) for v in ("auto", "mla16", "generic")]


@pytest.mark.parametrize("rotation,fmt,dtype,variant", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_mla_fp8_probe(rotation, fmt, dtype, variant):
    cfgs = M.cases(rotation)
    assert [c[:4] for c in cfgs] == M.CONFIGS and len({c[4] for c in cfgs}) == len(cfgs)
    descale = P.CODINGS[(rotation // 3) % 2]
    bad = run(dtype, variant, cfgs, stored(descale, fmt), descale)
    assert not bad, bad[:10]


@pytest.mark.parametrize("fmt,descale", [(E4, 0.25), (E5, 2.0)], ids=ids)
def test_every_split_count_meets_the_matrix_form(fmt, descale):
    """over the rotations of test_mla_fp8_probe each configuration meets some split counts; here the two-tile causal case meets all"""
    cfgs = [M.CONFIGS[3] + (n,) for n in M.SPLITS]
    bad = run(BF16, "mla16", cfgs, stored(descale, fmt), descale)
    assert not bad, bad[:10]


PAGED = [(64, "mla16", BF16, E4, 2.0), (128, "mla16", F16, E5, 0.25), (64, "mla16", F16, E5, 2.0), (16, "generic", BF16, E4, 0.25),
         (16, "generic", F16, E5, 2.0)]


@pytest.mark.parametrize("rotation,page,variant,dtype,fmt,descale", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_mla_fp8_probe_paged(rotation, page, variant, dtype, fmt, descale):
    """the fp8 latent cache behind a shuffled block table (scattered as bytes): the probe bars, every configuration"""
    pool, table = scatter(stored(descale, fmt).view(torch.uint8), page, 7 * page)
    bad = run(dtype, variant, M.cases(rotation + 3), pool.view(fmt), descale, block_table=table)
    assert not bad, bad[:10]
