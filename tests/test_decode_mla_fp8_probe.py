"""CPU proof that tests/mla_fp8_probe.py -- the exact-arithmetic probe tests/test_decode_mla_fp8_probe_gpu.py runs through MLA decode
over an fp8 latent cache (fa2_fwd_kvcache_mla_fp8) -- sees what it must:

  * under both codings (KV / 2 with descale 2, 4 KV with descale 0.25) every stored value is exactly representable in e4m3fn and in
    e5m2, and descale x stored is mla_probe's latent row again, bit for bit;
  * every planted error (the V descale left out of O, the K descale left out of the score or applied twice, the two halves of a
    16-element load or the element pairs of a word exchanged, a row fetched at the 16-bit row's byte stride, the last 64 columns taken
    from the 16-bit map's offsets) breaks a bar, computed with the reference restatement alone, in every sequence the plant changes
    -- on every configuration of the GPU grid, under both codings;
  * the un-planted restatement (emulate_split on the dequantised rows) breaks none, at every split count of the grid and what
    num_splits = 0 resolves to.

Bars: the decode probe's (oracle/fa2_decode_probe.violations) for 16-bit I/O -- one output ulp on O and L, exact zeros, exact empty
rows at any num_splits."""
import functools

import pytest
import torch

import mla_fp8_probe as P
import mla_probe as M
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from oracle import fa2_decode_probe as D

F16, BF16 = torch.float16, torch.bfloat16
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
B = len(M.LENS)


@functools.lru_cache(maxsize=None)
def cache():
    return M.latent_cache()


@functools.lru_cache(maxsize=None)
def stored(descale, fmt):
    return P.stored(cache(), descale, fmt)


def test_both_codings_are_exact_in_both_formats():
    KV = cache()
    assert P.F8 == (E4, E5) and set(P.CODINGS) == {2.0, 0.25}
    assert set(KV.unique().tolist()) == {float(v) for v in range(9)}
    for descale in P.CODINGS:
        for fmt in P.F8:
            KV8 = stored(descale, fmt)
            assert KV8.dtype == fmt and KV8.shape == KV.shape
            assert torch.equal(KV8.float().double(), KV / descale)                    # the stored value is the scaled row, exactly
            assert torch.equal(P.dequantised(KV8, descale), KV)                       # ... and descale x stored the probe's row
            for dt in (F16, BF16):                                                    # what staging writes to LDS
                assert torch.equal(KV8.to(dt).double(), KV / descale)
            K, V = P.seen(None, KV8, descale)
            assert torch.equal(K, KV) and torch.equal(V, M.value_of(KV))
    # a descale left out, or applied twice, is another number under either coding
    assert all(d != 1 and d * d != d for d in P.CODINGS)


def _auto(H, n_q, dtype):
    return _lib.kvcache_mla_num_splits(B, H, 1, n_q, M.S_K, 576, 512, convert_triton_dtype(dtype))


@pytest.mark.parametrize("k", range(len(M.CONFIGS)))
def test_unplanted_restatement_breaks_no_bar(k):
    H, n_q, causal, window = M.CONFIGS[k]
    keep = M.decode_keep(H, n_q, causal, window)
    descale, fmt = P.CODINGS[k % 2], P.F8[(k // 2) % 2]
    KV8 = stored(descale, fmt)
    for uniform in (False, True):
        Q = M.queries(H, n_q, uniform)
        for dt in (BF16, F16):
            if dt != BF16 and uniform:
                continue                                                        # (the count ratios: once)
            ref = M.mla_truth(Q, cache(), keep, dt)
            for n in sorted(set(M.SPLITS[1:]) | {_auto(H, n_q, dt)}):
                if dt != BF16 and n not in (1, 3, 128):
                    continue
                O, L = P.restate(Q, KV8, descale, keep, n, dt)
                assert O.shape[-1] == 512
                v = M.violations(O, L, *ref, dt, n > 1)
                assert not v, (M.CONFIGS[k], descale, fmt, uniform, dt, n, v)


@pytest.mark.parametrize("descale", P.CODINGS)
@pytest.mark.parametrize("k", range(len(M.CONFIGS)))
def test_every_plant_breaks_a_bar_in_every_sequence_it_changes(k, descale):
    """The planted restatement against the truth, each sequence judged on its own.  A plant changes a sequence where the fp64 truth
    of the planted computation differs from the un-planted truth; the scored probe must see it there, or the uniform one."""
    H, n_q, causal, window = M.CONFIGS[k]
    keep = M.decode_keep(H, n_q, causal, window)
    KV8 = stored(descale, P.F8[k % 2])
    seen_somewhere = set()
    for dt in (BF16, F16) if descale == P.CODINGS[0] else ((BF16, F16)[k % 2],):    # (the second coding: one I/O dtype per case)
        probes = {}
        for uniform in (False, True):
            Q = M.queries(H, n_q, uniform)
            probes[uniform] = (Q, M.mla_truth(Q, cache(), keep, dt))
        for name in P.PLANTS:
            changed = torch.zeros(B, dtype=torch.bool)
            caught = torch.zeros(B, dtype=torch.bool)
            for uniform, (Q, (O_ref, L_ref)) in probes.items():
                O_t, L_t = P.truth(Q, KV8, descale, keep, dt, name)
                ch = ((O_t != O_ref).reshape(B, -1).any(-1) | (L_t != L_ref).reshape(B, -1).any(-1))
                if not ch.any():
                    continue
                O_p, L_p = P.restate(Q, KV8, descale, keep, 1, dt, name)
                changed |= ch
                caught |= ch & D.violated(O_p, L_p, O_ref, L_ref, dt, False)
            missed = [M.LENS[b] for b in torch.nonzero(changed & ~caught).flatten().tolist()]
            assert not missed, (M.CONFIGS[k], descale, name, dt, missed)
            if changed.any():
                seen_somewhere.add(name)
    # every plant is a real error in some sequence of every configuration
    assert set(P.PLANTS) <= seen_somewhere, (M.CONFIGS[k], set(P.PLANTS) - seen_somewhere)
