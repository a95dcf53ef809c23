"""Exact-arithmetic probe for MLA decode over an fp8 latent cache (fa2_fwd_kvcache_mla_fp8).  TEST INFRASTRUCTURE ONLY:
tests/test_decode_mla_fp8_probe.py proves on the CPU that its bars see every planted error, tests/test_decode_mla_fp8_probe_gpu.py
runs it through the Python surface.  Device-agnostic.

It is tests/mla_probe.py (and through it oracle/fa2_decode_probe.py) with the latent rows STORED in fp8, reused by import.  The
probe's cache holds the integers 0..8 (score columns) and 0 / 1 (value code).  Under either coding of CODINGS -- stored as KV / 2
with descale 2, or as 4 KV with descale 0.25 -- every stored value is exactly representable in e4m3fn and in e5m2 (the largest
significand is 7 = 0b111: three bits, what e5m2 has), and descale x stored is the probe's row again, so the truth and every bar are
mla_probe's own.  Both descales differ from 1 and from each other's square, so a descale left out, or applied twice, moves every
score or every output.

restate() is the reference restatement: mla_probe.restate (oracle emulate_split) on the DEQUANTISED rows.  seen() is what a kernel
with one planted staging or descale error would hand to the same arithmetic:

  v_descale_dropped   the V descale left out of O
  k_descale_dropped   the K descale left out of the score
  k_descale_twice     the K descale applied twice
  halves_swapped      the two 8-element halves of a 16-element load exchanged (column c ^ 8)
  pairs_swapped       element pairs exchanged inside a 4-byte word (column c ^ 2)
  row_stride_16bit    a row fetched at the 16-bit row's byte stride (row 2 j for j, wrapping at the capacity)
  tail_16bit_offsets  the last 64 columns -- the second load pass of the 16-bit staging map -- taken from that map's byte offsets
                      1024.. of the row, which in 576-byte rows are columns 448..511 of the NEXT row"""
import torch

import mla_probe as M
from oracle import fa2_decode_probe as D

F8 = D.F8
CODINGS = (2.0, 0.25)  # kv_descale; the cache stores KV / kv_descale
PLANTS = ("v_descale_dropped", "k_descale_dropped", "k_descale_twice", "halves_swapped", "pairs_swapped", "row_stride_16bit",
          "tail_16bit_offsets")


def stored(KV, descale, fmt):
    """the latent rows as the fp8 cache holds them under kv_descale = descale"""
    return (KV / descale).float().to(fmt)


def dequantised(KV8, descale):
    """descale x float(KV8) in float64: what the call attends over"""
    return KV8.float().double() * descale


def seen(name, KV8, descale):
    """(K, V) in float64 as a kernel with the planted error `name` (None: a correct one) sees the cache"""
    X = KV8.float().double()
    kd = vd = descale
    cols = torch.arange(M.D_QK, device=X.device)
    if name == "v_descale_dropped":
        vd = 1.0
    elif name == "k_descale_dropped":
        kd = 1.0
    elif name == "k_descale_twice":
        kd = descale * descale
    elif name == "halves_swapped":
        X = X[..., cols ^ 8]
    elif name == "pairs_swapped":
        X = X[..., cols ^ 2]
    elif name == "row_stride_16bit":
        X = X[:, :, (2 * torch.arange(X.shape[2], device=X.device)) % X.shape[2]]
    elif name == "tail_16bit_offsets":
        Y = X.clone()
        Y[:, :, :-1, M.D_V:] = X[:, :, 1:, M.D_V - 64:M.D_V]
        Y[:, :, -1, M.D_V:] = 0
        X = Y
    else:
        assert name is None, name
    return kd * X, vd * X[..., :M.D_V]


def restate(Q, KV8, descale, keep, num_splits, dtype, plant=None, lens=M.LENS):
    """the reference restatement on what seen() hands it -> O (B, 1, R, 512), L (B, 1, R, 1) in the I/O dtype"""
    K, V = seen(plant, KV8, descale)
    return M.restate(Q, K, V, keep, lens, num_splits, dtype)


def truth(Q, KV8, descale, keep, dtype, plant=None):
    """fp64 O, L of the same"""
    K, V = seen(plant, KV8, descale)
    return M.truth(Q, K, V, keep, dtype)
