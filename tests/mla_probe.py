"""Exact-arithmetic probe for MLA decode (fa2_fwd_kvcache_mla): one shared latent row per key, d = 576, d_v = 512, V the first 512
columns of K.  TEST INFRASTRUCTURE ONLY: tests/test_decode_mla_probe.py proves on the CPU that its bars see every planted error,
tests/test_decode_mla_probe_gpu.py runs it through the Python surface.  Device-agnostic.

It is oracle/fa2_decode_probe.py for the aliased layout and reuses it by import (decode_keep, truth, emulate_split, violations,
LENS, SPLITS, S_K): scale = fp32(ln 2) makes c = 1, scores are integers in [0, 8], so P is a power of two and l and P V are exact
fp32 sums in any order, in any split.  H_kv = 1, u = b.  Because the value is a view of the key, ONE row carries both:

  * score columns: one per 16-column group that a 32x32x16 MFMA consumes, SCORE_COLS[k] = 16 k + 7 k mod 16 for k < 36 -- 32 below
    column 512, 4 in 512..575 -- so every k-step of the score carries weight and so do the rotary columns.  Row j holds
    (alpha_k (j + 5 u) + k // 6) mod 9 there, alpha_k = (1, 2, 4, 5, 7, 8)[k % 6]: the decode probe's keys.
  * Q: row r = hg N_q + qi of the group is one-hot at SCORE_COLS[(5 r + 32) mod 36] -- row 0 scores on a rotary column, the first
    16 rows already on both sides of column 512 and on k-step 0, 36 rows on every k-step; zero in every other column, so the
    value code never reaches a score.  uniform=True: Q = 0, O is a count ratio.
  * value-code columns: the 480 columns below 512 that are no score column hold the two-level one-hot of j + 17 u over w = 240.  A
    wrong, missing or repeated key lands in a column that must be exactly 0 or moves a count.
  * overlap: the 32 output columns that coincide with score columns are checked as well: O there is sum_j P_j K[j, c] / l, P a
    power of two in [2^-8, 1] and K <= 8 over at most 2560 keys, below 2^24 in units of 2^-8: exact in fp32.
  * rows at and behind N_k(b) are decoys: 8 in every score column (the largest score) and the value code of their own index.

restate() is the reference restatement: oracle/fa2_decode_probe.emulate_split (the split kernels and the combine launch in fp32)
on K = the latent rows and V = their first 512 columns, zero-padded to K's width for the emulation and cut again.  plant_*()
apply one error each to what the restatement reads or writes."""
import torch

from oracle import fa2_decode_probe as D
from oracle.fa2_decode_probe import LENS, S_K, SPLITS, decode_keep, emulate_split, truth, violations  # noqa: F401 (the probe's own)

D_QK, D_V = 576, 512
KSTEPS = D_QK // 16
SCORE_COLS = tuple(16 * k + (7 * k) % 16 for k in range(KSTEPS))
VALUE_COLS = tuple(c for c in range(D_V) if c not in SCORE_COLS)
W = len(VALUE_COLS) // 2
# (H, N_q, causal, window): one row tile, two, four, and a last partial tile (40 * 3 = 120 rows, 8 * 2 = 16)
CONFIGS = [(16, 1, False, None), (64, 1, False, None), (128, 1, False, None), (128, 2, True, None), (40, 3, True, (64, 0)),
           (8, 2, False, (100, 50))]
PLANTS = ("no_rope_columns", "drop_kstep", "v_from_column_64", "v_blocks_swapped", "second_tile_repeats_first", "plus32", "stale_leak",
          "drop_last_partial", "top_left")


def cases(rotation=0):
    """(H, N_q, causal, window, num_splits): every configuration under one split count, rotating with `rotation`"""
    return [cfg + (SPLITS[(k + rotation) % len(SPLITS)],) for k, cfg in enumerate(CONFIGS)]


def latent_cache(lens=LENS, s_k=S_K, device=None):
    """KV (B, 1, S_k, 576) in float64: score and value-code columns of every key, decoys from N_k(b) on"""
    B = len(lens)
    ar = lambda n: torch.arange(n, device=device)
    j = ar(s_k).view(1, 1, s_k, 1)
    u = ar(B).view(B, 1, 1, 1)
    k = ar(KSTEPS).view(1, 1, 1, KSTEPS)
    alpha = torch.tensor(D.ALPHA, device=device)[k % 6]
    sc = torch.tensor(SCORE_COLS, device=device)
    vc = torch.tensor(VALUE_COLS, device=device)
    KV = torch.zeros(B, 1, s_k, D_QK, dtype=torch.float64, device=device)
    n = torch.tensor(list(lens), device=device).view(B, 1, 1, 1)
    KV[..., sc] = torch.where(j >= n, 8.0, ((alpha * (j + 5 * u) + k // 6) % 9).double())
    gi = j + 17 * u
    KV.scatter_(-1, vc[gi % W], 1.0)
    KV.scatter_(-1, vc[W + (gi // W) % W], 1.0)
    return KV


def queries(H, n_q, uniform=False, B=len(LENS), device=None):
    """Q (B, 1, R, 576) in float64, row r = h N_q + qi of the one KV group"""
    R = H * n_q
    Q = torch.zeros(B, 1, R, D_QK, dtype=torch.float64, device=device)
    if not uniform:
        r = torch.arange(R, device=device)
        Q[:, :, r, torch.tensor(SCORE_COLS, device=device)[(5 * r + 32) % KSTEPS]] = 1.0
    return Q


def value_of(KV):
    """the value operand: the first 512 columns of the latent rows (a view)"""
    return KV[..., :D_V]


def mla_truth(Q, KV, keep, dtype, V=None):
    """fp64 O (B, 1, R, 512), L (B, 1, R, 1)"""
    return truth(Q, KV, value_of(KV) if V is None else V, keep, dtype)


def restate(Q, K, V, keep, lens, num_splits, dtype):
    """the reference restatement -> O (B, 1, R, 512), L (B, 1, R, 1) in the I/O dtype: emulate_split on V zero-padded to K's width
    (64 columns of exact zeros that are cut again: no other number changes)"""
    Vp = torch.zeros_like(K)
    Vp[..., :V.shape[-1]] = V
    O, L = emulate_split(Q, K, Vp, keep, lens, num_splits, dtype)
    return O[..., :V.shape[-1]].contiguous(), L


def planted(name, Q, KV, H, n_q, causal, window, fn, lens=LENS):
    """(O, L) of `fn(Q, K, V, keep)` -- the truth or the restatement, (B, 1, R, ...) layout -- under the planted error `name`:
      no_rope_columns            columns 512..575 left out of the score
      drop_kstep                 one 16-column k-step (columns 0..15: the one row 8 scores on, and with it every 36th row) left out
      v_from_column_64           V taken from columns 64..575
      v_blocks_swapped           value column blocks [128, 256) and [256, 384) exchanged in O
      second_tile_repeats_first  rows 64..127 answered with rows 0..63
      plus32                     rows r and r + 32 exchanged
      stale_leak, drop_last_partial, top_left   decode_keep's plants"""
    keep = decode_keep(H, n_q, causal, window, lens=lens, s_k=KV.shape[2], device=KV.device,
                       plant=name if name in ("stale_leak", "drop_last_partial", "top_left") else None)
    K, V = KV, value_of(KV)
    if name == "no_rope_columns":
        K = KV.clone()
        K[..., D_V:] = 0
    elif name == "drop_kstep":
        K = KV.clone()
        K[..., :16] = 0
    elif name == "v_from_column_64":
        V = KV[..., 64:]
    O, L = fn(Q, K, V, keep)
    R = H * n_q
    if name == "v_blocks_swapped":
        O = torch.cat([O[..., :128], O[..., 256:384], O[..., 128:256], O[..., 384:]], -1)
    elif name == "second_tile_repeats_first" and R > 64:
        n = min(R, 128) - 64
        O, L = O.clone(), L.clone()
        O[:, :, 64:64 + n], L[:, :, 64:64 + n] = O[:, :, :n], L[:, :, :n]
    elif name == "plus32":
        perm = D.row_permutation("plus32", H, n_q).to(O.device)
        O, L = O[:, :, perm], L[:, :, perm]
    return O, L
