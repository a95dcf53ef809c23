"""Exact-arithmetic probe for packed (ragged) queries over the latent cache (fa2_fwd_kvcache_mla_varlen: the VQ form of
fa2_decode_mla16.hip, the packed path of fa2_decode_combine.hip, the generic form).  TEST INFRASTRUCTURE ONLY:
tests/test_decode_mla_varlen_probe.py proves on the CPU that its bars see every planted error, tests/test_decode_mla_varlen_probe_gpu.py
runs it through the Python surface.  Device-agnostic.

It is tests/mla_probe.py (and through it oracle/fa2_decode_probe.py) on the ragged batch of tests/test_decode_mla_varlen_gpu.py,
reused by import: the latent rows, the one-hot queries, the value code, the fp64 truth, the fp32 restatement and the bars are
mla_probe's own, no arithmetic is added.  What is new is the batch and the layout:

  * sequence b has n_q(b) = N_Q[b] query tokens over N_K[b] keys; the cache of (sequence b, KV head h) is latent row set u = b H_kv
    + h of mla_probe.latent_cache, so a sequence or KV-head mix-up lands in value columns that must be 0;
  * every piece is computed PER SEQUENCE, with that sequence's own n_q(b), in mla_probe's layout: the KV heads as the batch axis,
    (H_kv, 1, R, ...) with R = g n_q(b) rows in the PROBE's order r = head * n_q + position (the order queries() colours the rows
    in);
  * the kernel flattens the same rows POSITION-major, rho = position * g + head, and cuts them into 64-row tiles.  kernel_rows()
    is the map between the two orders; pack() / group() go between the probe's layout and the call's (n_q, H, ...) rows, and
    packed() strings the sequences together to O (total_q, H, 512) and L (H, total_q).

planted() hands one error each to the truth or to the restatement.  The errors of the packed layout, modelled on the kernel's own
row map (tile t of a sequence holds the rows rho in [64 t, 64 t + 64), the positions [q0, q1) = [64 t / g, (64 t + 63) / g + 1)):

  head_major          row rho answered as head-major inside the group: (position, head) gets the row head' * n_q + position' = rho
  tile_local_mask     the band's row taken at position - q0 of the row's tile
  shift_from_max      the bottom-right shift N_k - max_seqlen_q
  neighbour_offset    the Q rows read from the next sequence's cu_seqlens_q offset on
  neighbour_len[_prev]   N_k of sequence b + 1 (b - 1), cyclically
  clip_first_tile     the first 64-key tile of a row tile's own band not read (kb0 from a q0 rounded up)
  clip_last_key       the last visible key of a row tile's own band not read (ke from a q1 one short)
  rotated_tile        the rows of tile t of sequence b answered by tile (t + b) % row_tiles(b): the x rotation on one side only
  plus32_packed       rows rho and rho + 32 of the kernel's order exchanged (mla_probe's plus32 exchanges them in the probe's)

and mla_probe.planted's own, per sequence: no_rope_columns, drop_kstep, v_from_column_64, v_blocks_swapped, plus32, stale_leak,
drop_last_partial, top_left.

Bars: mla_probe.violations unchanged.  The restatement's worst float32 error over this file's whole grid (every configuration,
both probes, every split count of SPLITS and what num_splits = 0 resolves to), measured by tests/test_decode_mla_varlen_probe.py
with oracle/fa2_decode_probe.fp32_ulp_error: 11.93 fp32 ulps on O and 1.29 on L (MEASURED_FP32_ULPS) -- inside the oracle's
SPLIT_MEASURED (12.8), and four times it, rounded up to a power of two, is the float32 split bar SPLIT_FP32_ULPS (64) as it stands."""
import functools

import torch

import mla_probe as M
from mla_probe import SCORE_COLS, SPLITS, decode_keep, latent_cache, mla_truth, queries, restate, violations  # noqa: F401
from oracle import fa2_decode_probe as D
from oracle.fa2_bwd_arith import band

# the ragged batch of tests/test_decode_mla_varlen_gpu.py
S_K = 2560
N_Q = [0, 1, 3, 2, 5, 17, 1, 70, 64]
N_K = [100, 0, 2, 65, 64, 1000, S_K, 300, 64]
B, TOTAL, MAX_Q = len(N_Q), sum(N_Q), max(N_Q)
CU = [0] + torch.tensor(N_Q).cumsum(0).tolist()
WINDOWS = (None, (64, 0), (100, 50), (0, 0))
# (g, H_kv, causal, window), that file's: a tile spanning many positions (g 1, 5, 16), exactly one (g 64), smaller than one
# position's heads (g 128), cutting a position (g 5, 40), two KV heads
CONFIGS = [(1, 1, True, None), (5, 1, False, (64, 0)), (16, 1, True, (100, 50)), (40, 1, False, None), (64, 1, True, (0, 0)),
           (128, 1, False, (100, 50)), (16, 2, True, (64, 0)), (128, 1, True, None)]
MEASURED_FP32_ULPS = 11.93       # on O; 1.29 on L (the module docstring; re-measured and printed by the CPU proof)
LAYOUT_PLANTS = ("head_major", "tile_local_mask", "shift_from_max", "neighbour_offset", "neighbour_len", "neighbour_len_prev",
                 "clip_first_tile", "clip_last_key", "rotated_tile", "plus32_packed")
MLA_PLANTS = ("no_rope_columns", "drop_kstep", "v_from_column_64", "v_blocks_swapped", "plus32", "stale_leak", "drop_last_partial",
              "top_left")
PLANTS = LAYOUT_PLANTS + MLA_PLANTS
# the plants that only move finished rows or columns: planted() calls `fn` on the un-planted inputs, so a caller may hand it a stored result
OUTPUT_PLANTS = ("head_major", "rotated_tile", "plus32_packed", "v_blocks_swapped", "plus32")
ROW_TILE = 64


def cases(rotation=0):
    """(g, H_kv, causal, window, num_splits): every configuration under one split count, rotating with `rotation`"""
    return [cfg + (SPLITS[(k + rotation) % len(SPLITS)],) for k, cfg in enumerate(CONFIGS)]


def split_formula(g, h_kv):
    """what num_splits = 0 resolves to on the matrix form for this batch: the formula of tests/test_decode_mla_varlen_host.py (one
    wave of 256 workgroups, splits of at least eight key tiles)"""
    base = h_kv * min(B * -(-g * MAX_Q // ROW_TILE), -(-g * TOTAL // ROW_TILE) + B)
    return 1 if base >= 256 else max(1, min(-(-256 // base), -(-S_K // 64) // 8, 128))


@functools.lru_cache(maxsize=None)
def cache(h_kv=1, device=None):
    """the latent rows (B, H_kv, S_k, 576) in float64, decoys behind N_K[b]: (sequence b, KV head h) is row set u = b H_kv + h"""
    return latent_cache(lens=[n for n in N_K for _ in range(h_kv)], s_k=S_K, device=device).view(B, h_kv, S_K, M.D_QK)


def seq_cache(h_kv, b, device=None):
    """the rows of sequence b in mla_probe's layout, the KV heads as the batch: (H_kv, 1, S_k, 576)"""
    return cache(h_kv, device)[b].unsqueeze(1)


def seq_queries(g, n_q, uniform, h_kv=1, device=None):
    """mla_probe.queries of one sequence, the same for each of its KV heads: (H_kv, 1, R, 576), row r = head * n_q + position"""
    return queries(g, n_q, uniform, B=1, device=device).expand(h_kv, 1, g * n_q, M.D_QK)


def kernel_rows(g, n_q, device=None):
    """the probe's row r = head * n_q + position of each of the kernel's rows rho = position * g + head"""
    rho = torch.arange(g * n_q, device=device)
    return (rho % g) * n_q + rho // g


def probe_rows(g, n_q, device=None):
    """the kernel's row rho = position * g + head of each of the probe's rows r = head * n_q + position"""
    r = torch.arange(g * n_q, device=device)
    return (r % n_q) * g + r // n_q


def pack(x, g, n_q):
    """(H_kv, 1, R, ...) in the probe's order -> the call's (n_q, H, ...), H = h_kv g + head"""
    h_kv = x.shape[0]
    k = x[:, 0, kernel_rows(g, n_q, x.device)]                      # (H_kv, position, head, ...)
    return k.reshape(h_kv, n_q, g, *x.shape[3:]).transpose(0, 1).reshape(n_q, h_kv * g, *x.shape[3:])


def group(x, g):
    """the call's (n_q, H, ...) -> (H_kv, 1, R, ...) in the probe's order"""
    n_q, H = x.shape[:2]
    k = x.reshape(n_q, H // g, g, *x.shape[2:]).transpose(0, 1).reshape(H // g, n_q * g, *x.shape[2:])
    return k[:, probe_rows(g, n_q, x.device)].unsqueeze(1)


def packed_queries(g, h_kv, uniform, device=None):
    """the probe's Q of every sequence, packed (total_q, H, 576)"""
    return torch.cat([pack(seq_queries(g, n, uniform, h_kv, device), g, n) for n in N_Q if n])


def packed(per_seq, g):
    """[(O_b, L_b) or None] in the probe's layout -> O (total_q, H, 512), L (H, total_q) as the call returns them"""
    O = torch.cat([pack(r[0], g, n) for r, n in zip(per_seq, N_Q) if n])
    L = torch.cat([pack(r[1], g, n) for r, n in zip(per_seq, N_Q) if n])
    return O, L[..., 0].t().contiguous()


def _from_kernel_order(keep_k, g, n_q, h_kv):
    """a (R, S_k) mask whose rows are in the kernel's order -> (H_kv, 1, R, S_k) in the probe's"""
    return keep_k[probe_rows(g, n_q, keep_k.device)].expand(h_kv, 1, g * n_q, keep_k.shape[-1])


def seq_keep(g, h_kv, b, causal, window, plant=None, device=None, max_q=MAX_Q):
    """(H_kv, 1, R, S_k) visible (row, key) pairs of sequence b; plant: a mask or key-range error of the packed layout"""
    n_q, n_k = N_Q[b], N_K[b]
    if plant in ("neighbour_len", "neighbour_len_prev"):
        n_k = N_K[(b + (1 if plant == "neighbour_len" else -1)) % B]
        plant = None
    keep = decode_keep(g, n_q, causal, window, lens=[n_k] * h_kv, s_k=S_K, device=device)
    if plant is None:
        return keep
    base = keep[0, 0, :n_q]                                          # (n_q, S_k): the rows of one head
    rho = torch.arange(g * n_q, device=device)
    pos = rho // g
    if plant == "shift_from_max":
        m = band(max_q, n_k, causal, window, device)
        base = torch.zeros_like(base)
        base[:, :n_k] = m[:n_q]
        keep_k = base[pos]
    elif plant == "tile_local_mask":
        keep_k = base[pos - rho // ROW_TILE * ROW_TILE // g]
    elif plant in ("clip_first_tile", "clip_last_key"):
        keep_k = base[pos].clone()
        for r0 in range(0, g * n_q, ROW_TILE):                       # the keys the band of the tile's own rows touches
            rows = keep_k[r0:r0 + ROW_TILE]
            cols = torch.nonzero(rows.any(0)).flatten()
            if cols.numel():
                first, last = int(cols[0]), int(cols[-1])
                if plant == "clip_first_tile":
                    rows[:, first // 64 * 64:first // 64 * 64 + 64] = False
                else:
                    rows[:, last] = False
    else:
        raise ValueError(plant)
    return _from_kernel_order(keep_k, g, n_q, h_kv)


def row_source(name, g, n_q, b):
    """the probe-order source row of each of the R rows under a planted row mix-up of the kernel's layout"""
    R = g * n_q
    if name == "head_major":
        return probe_rows(g, n_q)                                    # (position, head) gets the row whose probe index is rho
    rho = torch.arange(R)
    if name == "rotated_tile":
        T = -(-R // ROW_TILE)
        src_k = (((rho // ROW_TILE + b) % T) * ROW_TILE + rho % ROW_TILE).clamp(max=R - 1)     # padding rows repeat the last row
    elif name == "plus32_packed":
        src_k = D.row_permutation("plus32", g, n_q)
    else:
        raise ValueError(name)
    return kernel_rows(g, n_q)[src_k[probe_rows(g, n_q)]]


def seq_truth(g, h_kv, b, causal, window, uniform, dtype, device=None):
    """the fp64 truth of sequence b (n_q(b) > 0) -> O (H_kv, 1, R, 512), L (H_kv, 1, R, 1)"""
    return mla_truth(seq_queries(g, N_Q[b], uniform, h_kv, device), seq_cache(h_kv, b, device),
                     seq_keep(g, h_kv, b, causal, window, device=device), dtype)


def ragged_truth(g, h_kv, causal, window, uniform, dtype, device=None):
    """[(O_b, L_b) or None] per sequence"""
    return [seq_truth(g, h_kv, b, causal, window, uniform, dtype, device) if N_Q[b] else None for b in range(B)]


def restate_counts(Q, K, V, keep, lens, counts, dtype):
    """{num_splits: mla_probe.restate(Q, K, V, keep, lens, num_splits, dtype)} on one set of scores"""
    Vp = torch.zeros_like(K)
    Vp[..., :V.shape[-1]] = V
    return {n: (O[..., :V.shape[-1]].contiguous(), L) for n, (O, L) in D.emulate_splits(Q, K, Vp, keep, lens, tuple(counts), dtype).items()}


def seq_restate(g, h_kv, b, causal, window, uniform, dtype, counts, device=None):
    """the reference restatement of sequence b at each split count of `counts` -> {n: (O, L)} in the I/O dtype"""
    KV = seq_cache(h_kv, b, device)
    return restate_counts(seq_queries(g, N_Q[b], uniform, h_kv, device), KV, M.value_of(KV), seq_keep(g, h_kv, b, causal, window, device=device),
                          [N_K[b]] * h_kv, counts, dtype)


def planted(name, g, h_kv, b, causal, window, uniform, fn, device=None):
    """(O, L) of `fn(Q, K, V, keep)` -- the truth or the restatement, (H_kv, 1, R, ...) -- for sequence b under the planted error
    `name` (None: no error)"""
    n_q, n_k = N_Q[b], N_K[b]
    Q, KV = seq_queries(g, n_q, uniform, h_kv, device), seq_cache(h_kv, b, device)
    if name in MLA_PLANTS:
        return M.planted(name, Q, KV, g, n_q, causal, window, fn, lens=[n_k] * h_kv)
    if name == "neighbour_offset":
        tok = (CU[b + 1] + torch.arange(n_q, device=device)) % TOTAL
        Q = group(packed_queries(g, h_kv, uniform, device)[tok], g)
    keep_plant = name if name in ("tile_local_mask", "shift_from_max", "neighbour_len", "neighbour_len_prev", "clip_first_tile",
                                  "clip_last_key") else None
    O, L = fn(Q, KV, M.value_of(KV), seq_keep(g, h_kv, b, causal, window, keep_plant, device))
    if name in ("head_major", "rotated_tile", "plus32_packed"):
        src = row_source(name, g, n_q, b).to(O.device)
        O, L = O[:, :, src], L[:, :, src]
    elif name is not None and keep_plant is None and name != "neighbour_offset":
        raise ValueError(name)
    return O, L
