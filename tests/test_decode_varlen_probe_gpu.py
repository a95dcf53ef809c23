"""The exact-arithmetic probe (oracle/fa2_decode_probe.py) through fa2_fwd_kvcache_varlen on the ragged batch of
tests/test_decode_varlen_gpu.py: O within one output ulp of the fp64 truth, exact zeros where no visible key writes, L within one
ulp, empty rows O = 0 and L = +inf -- for both kernel forms, both 16-bit dtypes, float32 / float64 on the VALU form, both fp8
formats, page sizes 16 / 64 / 128.  Random data cannot see P times the wrong V tile at these lengths; this file pins which keys a
query tile reads and which mask each of its rows gets.  tests/test_decode_varlen_host.py shows on the CPU that each error a
query-tiled kernel over packed rows can make fails these bars in every sequence it changes."""
import functools

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D
from test_decode_probe_gpu import scatter
from test_decode_varlen_host import B, CU, H_KV, MAX_Q, N_K, N_Q, PROBE_CONFIGS, S_K, pack_rows, ragged_cache, ragged_truth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
E4, E5 = D.F8
TOTAL = sum(N_Q)

ids = lambda x: str(x).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def case(d, g, causal, window, uniform, c64):
    """packed Q (total_q, H, d) in float64 and the fp64 truth O (total_q, H, d), L (total_q, H, 1) of one configuration: computed
    once, shared by every variant, dtype and cache form, never modified (c64: float64 I/O's c = 1 + 2.7e-9)"""
    per = [r for r in ragged_truth(g, d, causal, window, uniform, F64 if c64 else F32, device=DEV) if r is not None]
    nqs = [n for n in N_Q if n]
    return tuple(torch.cat([pack_rows(r[k], g, n) for r, n in zip(per, nqs)]) for k in (0, 2, 3))


def cases(rotation):
    """(g, causal, window, num_splits): every configuration under two split counts, all seven over the configurations"""
    out = [cfg + (D.SPLITS[(2 * k + j + rotation) % len(D.SPLITS)],) for k, cfg in enumerate(PROBE_CONFIGS) for j in (0, 1)]
    assert {c[3] for c in out} == set(D.SPLITS)
    return out


def run(dtype, variant, d, cfgs, K, V, **kw):
    bad = []
    cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
    lens = torch.tensor(N_K, dtype=torch.int32, device=DEV)
    for g, causal, window, n in cfgs:
        resolved = n or _lib.kvcache_varlen_num_splits(B, g * H_KV, H_KV, TOTAL, MAX_Q, S_K, d, convert_triton_dtype(dtype))
        for uniform in (False, True):
            Q, O_ref, L_ref = case(d, g, causal, window, uniform, dtype == F64)
            O, L = fa.flash_attention_varlen_kvcache_forward(Q.to(dtype), K, V, cu, MAX_Q, lens, DEV, causal=causal, scale=D.SCALE,
                                                             window=window, num_splits=n, variant=variant, **kw)
            assert O.shape == Q.shape and O.dtype == dtype and L.dtype == dtype
            v = D.violations(O, L.t().unsqueeze(-1).contiguous(), O_ref, L_ref, dtype, resolved > 1)
            if v:
                worst = [b for b in range(B) if N_Q[b] and D.violations(O[CU[b]:CU[b + 1]], L[:, CU[b]:CU[b + 1]].t().unsqueeze(-1).contiguous(),
                                                                      O_ref[CU[b]:CU[b + 1]], L_ref[CU[b]:CU[b + 1]], dtype, resolved > 1)]
                bad.append(((g, causal, window, n, resolved), "uniform" if uniform else "scored", v, "sequences", worst))
    return bad


FWD = [(dt, v, d) for dt in (F16, BF16) for v in ("auto", "generic", "mfma16") for d in (64, 128)]
FWD += [(dt, "generic", d) for dt in (F32, F64) for d in (64, 40)]


@pytest.mark.parametrize("rotation,dtype,variant,d", [(k,) + c for k, c in enumerate(FWD)], ids=ids)
def test_ragged_probe(rotation, dtype, variant, d):
    K, V = (t.to(dtype) for t in ragged_cache(d, DEV))
    bad = run(dtype, variant, d, cases(rotation), K, V)
    assert not bad, bad[:10]


def descales():
    return {"k_descale": torch.full((B, H_KV), D.K_DESCALE, device=DEV), "v_descale": torch.full((B, H_KV), D.V_DESCALE, device=DEV)}


FP8 = [(fmt, dt, v, d) for fmt in (E4, E5) for dt, v, d in ((BF16, "mfma16", 128), (F16, "mfma16", 64), (BF16, "generic", 64), (F16, "generic", 128))]


@pytest.mark.parametrize("rotation,fmt,dtype,variant,d", [(k,) + c for k, c in enumerate(FP8)], ids=ids)
def test_ragged_probe_fp8_cache(rotation, fmt, dtype, variant, d):
    """K8 = K / 2 under k_descale 2, V8 = 4 V under v_descale 0.25: the same truth"""
    K8, V8 = D.fp8_cache(*ragged_cache(d, DEV), fmt)
    bad = run(dtype, variant, d, cases(rotation), K8, V8, **descales())
    assert not bad, bad[:10]


PAGED = [(64, "mfma16", BF16, None, 128), (128, "mfma16", F16, None, 64), (16, "generic", BF16, None, 64),
         (64, "mfma16", F16, E4, 64), (128, "mfma16", BF16, E5, 128), (16, "generic", F16, E4, 128), (16, "auto", F32, None, 40)]


@pytest.mark.parametrize("rotation,page,variant,dtype,fmt,d", [(k,) + c for k, c in enumerate(PAGED)], ids=ids)
def test_ragged_probe_paged(rotation, page, variant, dtype, fmt, d):
    """the probe's cache behind a shuffled block table, decoy rows behind N_k(b) and in the spare pages"""
    K, V = D.fp8_cache(*ragged_cache(d, DEV), fmt) if fmt else (t.to(dtype) for t in ragged_cache(d, DEV))
    Kp, Vp, table = scatter(K, V, page, 7 * page + d)
    bad = run(dtype, variant, d, cases(rotation), Kp, Vp, block_table=table, **(descales() if fmt else {}))
    assert not bad, bad[:10]
