"""Exact-arithmetic probe for the KV-cache decode kernels (fa2_fwd_kvcache*, split-KV and the combine launch).

TEST INFRASTRUCTURE ONLY (tests/test_decode_probe.py proves on the CPU that its bars see every planted decode error;
tests/test_decode_probe_gpu.py runs it through every decode form: 16-bit, fp8 cache, paged, layouts).  Device-agnostic.

It is oracle/fa2_mask_probe.py brought to decode: scale = fp32(ln 2) makes c = 1, the inputs below make every score an integer
in [0, 8], so P is a power of two and l and P V are exact fp32 sums in any order, in any split.  For one (b, h_kv), u = b H_kv + h_kv:
  * K[j, c] = (alpha_c (j + 5 u) + c // 6) mod 9 for c < min(54, d), alpha_c = (1, 2, 4, 5, 7, 8)[c % 6], the rest 0: integers in
    [0, 8], exact in bf16, f16, e4m3fn and e5m2.
  * Q: row r = hg N_q + qi of the KV group (R = g N_q rows) is one-hot at column r mod min(54, d), so the rows of one group carry
    different score patterns and a row that lands in another row's place shows.  uniform=True: Q = 0, O is a count ratio.
  * V: the mask probe's two-level one-hot of j + 17 u over w = d // 2.  A wrong, missing or repeated key lands in a column that must
    be exactly 0 or moves a count; a wrong KV head or sequence shows in its own columns.
  * rows at and behind N_k(b) are decoys, not zeros: K = 8 in every column (the largest score) and the V one-hots of their own
    indices, so a leaked stale row moves a count and cannot vanish.
  * fp8 cache: K8 = K / 2 under k_descale 2, V8 = 4 V under v_descale 0.25: exact in both formats, c kd = 2 exact; a dropped or
    swapped descale gives non-integer scores or an output off by a power of two.

emulate_split() restates the split kernels and fa2_decode_combine.hip in fp32: the split rule of fa2_decode.h (chunk
ceil(N_k / num_splits) rounded up to 64), per split P rounded to the I/O dtype before P V, O_s = o (1 / l), L_s = m + log2 l (an
empty split: 0 and -inf), then w_s = 2^(L_s - m), O = sum w_s O_s (1 / sum w_s), L = m + log2 sum w_s and the cast.  The bars must
accept it.

Bars (violations()):
  * f16 / bf16 I/O, 16-bit or fp8 cache, any num_splits: fa2_mask_probe.violations unchanged -- |O - O_ref| <= 1 ulp_io, O == 0
    exactly where the truth is 0, L within 1 ulp_io, empty rows O = 0 and L = +inf exactly.
  * f32 I/O, one split: the mask probe's 4 fp32 ulps.  f64 I/O, one split: its 1e-6.
  * f32 and f64 I/O, split (the partials are fp32 whatever the I/O dtype; L_s, rounded to fp32 at magnitudes up to 2^4, is the
    exponent of a weight): SPLIT_FP32_ULPS fp32 ulps of the truth.  Measured, never fitted to a kernel: the worst error of
    emulate_split against the fp64 truth over the whole f32 / f64 grid of the GPU test (every configuration, both probes, d 64
    and 40, num_splits 2, 3, 7, 16, 128) is 12.75 fp32 ulps on O and 1.09 on L, SPLIT_MEASURED = 12.8
    (tests/test_decode_probe.py re-measures it); the bar is 4 times that rounded up to a power of two, 64.  The margin covers
    the hardware's exp2 and log2 at 1 ulp where torch's CPU ones are nearer half, and the combine's summation order.  The
    exact-zero rule stays.

On the MI355X every decode form passes these bars unchanged: exp2 at integer arguments is exact, the f16 and bf16 matrix
instructions flush nothing the probe uses, and the combine's 2^(L_s - m) stays inside the split bar.
"""
import math

import torch

from oracle import fa2_mask_probe as P
from oracle.fa2_bwd_arith import band, c_log2e
from oracle.fa2_mask_probe import SCALE, ulp

KEY_TILE = 64                    # FA2_KVCACHE_KEY_TILE
SPLIT_MEASURED = 12.8            # worst fp32-ulp error of emulate_split over the f32 / f64 grid (module docstring)
SPLIT_FP32_ULPS = 64.0           # 4 * SPLIT_MEASURED, rounded up to a power of two

# the GPU grid (tests/test_decode_probe_gpu.py) and the CPU proof (tests/test_decode_probe.py) walk the same cases
S_K = 2560
H_KV = 2
LENS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 513, 1025, 1100, 2049, 2500)
SPLITS = (0, 1, 2, 3, 7, 16, 128)
# (g, N_q, causal, window)
CONFIGS = [(4, 1, False, None), (1, 2, True, None), (8, 5, False, (64, 0)), (32, 1, False, (100, 50)), (4, 16, True, (64, 0)),
           (32, 2, False, None), (8, 2, True, (100, 50)), (2, 3, True, (0, 0))]
VALU_CONFIGS = [(8, 10, True, None), (1, 33, True, (17, 3))]     # 80 rows; three 16-row tiles
ALPHA = (1, 2, 4, 5, 7, 8)
F8 = (torch.float8_e4m3fn, torch.float8_e5m2)
K_DESCALE, V_DESCALE = 2.0, 0.25

KEEP_PLANTS = ("stale_leak", "drop_tile", "drop_last_partial", "top_left", "neighbour_len", "neighbour_len_prev")
INPUT_PLANTS = ("v_tile_swap", "kv_head_mod")
ROW_PLANTS = ("row_transposed", "next_row", "plus32", "pair_swap")
FP8_PLANTS = ("descale_dropped_k", "descale_dropped_v", "descales_swapped")


def cases(rotation=0, valu=False):
    """(g, N_q, causal, window, num_splits): every configuration under one split count, the split counts rotating with `rotation`
    (the GPU test passes the index of its parametrised case, so a configuration meets other split counts from case to case)"""
    cfgs = CONFIGS + (VALU_CONFIGS if valu else [])
    return [cfg + (SPLITS[(k + rotation) % len(SPLITS)],) for k, cfg in enumerate(cfgs)]


def probe_cache(d, lens=LENS, s_k=S_K, h_kv=H_KV, device=None):
    """K, V (B, H_kv, S_k, d) in float64: the probe's keys and values, decoys from N_k(b) on"""
    B = len(lens)
    nc, w = min(54, d), d // 2
    ar = lambda n: torch.arange(n, device=device)
    j = ar(s_k).view(1, 1, s_k, 1)
    u = (ar(B).view(B, 1) * h_kv + ar(h_kv).view(1, h_kv)).view(B, h_kv, 1, 1)
    c = ar(nc).view(1, 1, 1, nc)
    alpha = torch.tensor(ALPHA, device=device)[c % 6]
    K = torch.zeros(B, h_kv, s_k, d, dtype=torch.float64, device=device)
    K[..., :nc] = ((alpha * (j + 5 * u) + c // 6) % 9).double()
    n = torch.tensor(list(lens), device=device).view(B, 1, 1, 1)
    K = torch.where(j >= n, 8.0, K)
    gi = j + 17 * u
    V = torch.zeros(B, h_kv, s_k, d, dtype=torch.float64, device=device)
    V.scatter_(-1, gi % w, 1.0)
    V.scatter_(-1, w + (gi // w) % w, 1.0)
    return K, V


def probe_queries(g, n_q, d, uniform=False, B=len(LENS), h_kv=H_KV, device=None):
    """Q (B, H_kv, R, d) in float64, row r = hg N_q + qi of each KV group"""
    R = g * n_q
    Q = torch.zeros(B, h_kv, R, d, dtype=torch.float64, device=device)
    if not uniform:
        r = torch.arange(R, device=device)
        Q[:, :, r, r % min(54, d)] = 1.0
    return Q


def to_heads(x, g, n_q):
    """(B, H_kv, R, ...) rows of the KV groups -> (B, H, N_q, ...), h = h_kv g + hg"""
    return x.reshape(x.shape[0], x.shape[1] * g, n_q, *x.shape[3:])


def to_groups(x, g, n_q):
    """(B, H, N_q, ...) -> (B, H_kv, R, ...)"""
    return x.reshape(x.shape[0], x.shape[1] // g, g * n_q, *x.shape[3:])


def decode_keep(g, n_q, causal, window, lens=LENS, s_k=S_K, plant=None, device=None):
    """(B, 1, R, S_k) visible (row, key) pairs: fa2_bwd_arith.band over the first N_k(b) keys, bottom-right aligned per sequence.
    plant (tests only): stale_leak -- the band runs on into key N_k; drop_tile -- the last full 64-key tile is not read;
    drop_last_partial -- the keys from N_k - N_k % 64 on are not read; top_left -- top-left alignment; neighbour_len[_prev] --
    sequence b runs with the length of b + 1 (b - 1), cyclically."""
    B = len(lens)
    if plant == "neighbour_len":
        lens = [lens[(b + 1) % B] for b in range(B)]
    elif plant == "neighbour_len_prev":
        lens = [lens[(b - 1) % B] for b in range(B)]
    keep = torch.zeros(B, 1, g * n_q, s_k, dtype=torch.bool, device=device)
    for b, nk in enumerate(lens):
        m = band(n_q, nk, causal, window, device, plant="top_left" if plant == "top_left" else None)
        full = torch.zeros(n_q, s_k, dtype=torch.bool, device=device)
        full[:, :nk] = m
        if plant == "stale_leak" and nk < s_k:
            full[:, nk] = full[:, nk - 1] if nk else True
        elif plant == "drop_tile" and nk >= KEY_TILE:
            t = nk // KEY_TILE - 1
            full[:, t * KEY_TILE:(t + 1) * KEY_TILE] = False
        elif plant == "drop_last_partial":
            full[:, nk - nk % KEY_TILE:] = False
        keep[b, 0] = full.repeat(g, 1)
    return keep


def by_extent(fn, Q, K, V, keep, lens=None, from_zero=False):
    """fn(Q, K, V, keep[, lens]) -> tensors with a leading sequence axis, evaluated on groups of sequences whose visible keys span
    similar extents, each on the slice of keys it sees (from_zero: from key 0 on, in whole 64-key tiles): the same numbers as one
    call over the whole capacity -- a key no row sees contributes to nothing -- at a fraction of the work for the short
    sequences"""
    B, S = keep.shape[0], keep.shape[-1]
    seen = keep.any(-2).reshape(B, S)
    j = torch.arange(S, device=keep.device)
    hi = torch.where(seen, j + 1, 0).amax(-1).tolist()
    lo = torch.where(seen, j, S).amin(-1).tolist()
    groups = {}
    for b in range(B):
        first = 0 if from_zero or not hi[b] else lo[b]
        W = min(S, max(KEY_TILE, 1 << max(hi[b] - first - 1, 0).bit_length()))
        groups.setdefault(W, []).append((b, min(first, S - W)))
    outs = None
    for W, members in groups.items():
        bs = [b for b, _ in members]
        cut = lambda t: torch.stack([t[b, ..., first:first + W, :] for b, first in members])
        args = (Q[bs], cut(K), cut(V), torch.stack([keep[b, ..., first:first + W] for b, first in members]))
        res = fn(*args, [lens[b] for b in bs]) if lens is not None else fn(*args)
        if outs is None:
            outs = [torch.empty((B,) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device) for r in res]
        for o, r in zip(outs, res):
            o[bs] = r
    return tuple(outs)


def truth(Q, K, V, keep, dtype, scale=SCALE):
    """fa2_mask_probe.truth: fp64 O (B, H_kv, R, d) and L (B, H_kv, R, 1) with the kernel's own c; rows without a visible key:
    O = 0, L = +inf"""
    return by_extent(lambda q, k, v, kp: P.truth(q, k, v, kp, dtype, scale), Q, K, V, keep)


def v_tile_swap(V, lens=LENS, full_tiles=False):
    """V with two adjacent 64-key tiles of every sequence exchanged: the tile of key N_k - 1 and the one before it (full_tiles: the
    last two tiles wholly below N_k)"""
    V = V.clone()
    for b, nk in enumerate(lens):
        t1 = nk // KEY_TILE - 1 if full_tiles else (nk - 1) // KEY_TILE
        if t1 >= 1 and (t1 + 1) * KEY_TILE <= V.shape[2]:
            a, c, e = (t1 - 1) * KEY_TILE, t1 * KEY_TILE, (t1 + 1) * KEY_TILE
            V[b, :, a:c], V[b, :, c:e] = V[b, :, c:e].clone(), V[b, :, a:c].clone()
    return V


def kv_head_mod_truth(Q, K, V, keep, dtype, g, n_q):
    """the truth of a kernel that takes KV head h % H_kv instead of h // g -> O, L in the (B, H_kv, R, ...) layout"""
    B, h_kv, R, d = Q.shape
    H = h_kv * g
    rows = Q.reshape(B, 1, h_kv * R, d)                                          # every row of the call against every KV head
    O, L = truth(rows, K, V, keep.repeat(1, 1, h_kv, 1), dtype)                  # (B, H_kv, H N_q, ...)
    sel = torch.arange(H, device=Q.device) % h_kv
    pick = lambda t: to_groups(t.view(B, h_kv, H, n_q, -1)[:, sel, torch.arange(H, device=Q.device)], g, n_q)
    return pick(O), pick(L)


def row_permutation(name, g, n_q):
    """source row of each of the R rows of a group under a planted row mix-up (an index tensor; the identity: no plant)"""
    R = g * n_q
    r = torch.arange(R)
    if name == "row_transposed":
        return (r % n_q) * g + r // n_q
    if name == "next_row":
        return (r + 1) % R
    if name == "plus32":
        return torch.where(r + 32 < R, r + 32, torch.where(r >= 32, r - 32, r))
    if name == "pair_swap":
        return torch.where((r ^ 1) < R, r ^ 1, r)
    raise ValueError(name)


def fp8_plant(name, K, V):
    """the dequantised cache a kernel sees that drops a descale or swaps the two (K8 = K / 2, V8 = 4 V)"""
    K8, V8 = K / K_DESCALE, V / V_DESCALE
    kd, vd = {"descale_dropped_k": (1.0, V_DESCALE), "descale_dropped_v": (K_DESCALE, 1.0),
              "descales_swapped": (V_DESCALE, K_DESCALE)}[name]
    return K8 * kd, V8 * vd


def fp8_cache(K, V, fmt):
    """(K8, V8) in `fmt`, to be called with k_descale = K_DESCALE, v_descale = V_DESCALE"""
    return (K / K_DESCALE).float().to(fmt), (V / V_DESCALE).float().to(fmt)


def split_chunk(n_k, num_splits):
    """the split rule of fa2_decode.h: split s of a sequence of n_k keys covers [s c, (s + 1) c)"""
    return -(-(-(-n_k // num_splits)) // KEY_TILE) * KEY_TILE


def emulate_split(Q, K, V, keep, n_k, num_splits, dtype):
    """a valid implementation of the split decode: Q (B, H_kv, R, d), K, V (B, H_kv, S_k, d), keep (B, 1, R, S_k), n_k the B
    lengths -> (O, L) in the I/O dtype.  S, l and P V per split in fp32 (float64 I/O: in double, as the VALU form does), the
    partials O_s, L_s in fp32, the combine in fp32, the cast; num_splits = 1 is fa2_mask_probe.emulate."""
    return emulate_splits(Q, K, V, keep, n_k, (num_splits,), dtype)[num_splits]


def emulate_splits(Q, K, V, keep, n_k, counts, dtype):
    """{num_splits: emulate_split(...)} for several split counts on one set of scores.  Evaluated over the tiles that hold a
    visible key (by_extent): the tiles past them are empty splits or parts of splits, O_s = 0 and w_s = 0, and change no bit."""
    res = by_extent(lambda q, k, v, kp, n: _emulate_splits(q, k, v, kp, n, counts, dtype), Q, K, V, keep, n_k, from_zero=True)
    return {n: (res[2 * i], res[2 * i + 1]) for i, n in enumerate(counts)}


def _emulate_splits(Q, K, V, keep, n_k, counts, dtype):
    f = torch.float64 if dtype == torch.float64 else torch.float32
    B, h_kv, R, d = Q.shape
    S = K.shape[2]
    T = -(-S // KEY_TILE)
    dev = Q.device
    c = c_log2e(SCALE, dtype)
    q, k, v = (t.to(f) for t in (Q, K, V))
    Sc = (torch.matmul(q, k.transpose(-1, -2)) * c).masked_fill(~keep, -math.inf)
    if T * KEY_TILE != S:
        Sc = torch.nn.functional.pad(Sc, (0, T * KEY_TILE - S), value=-math.inf)
        v = torch.nn.functional.pad(v, (0, 0, 0, T * KEY_TILE - S))
    St = Sc.view(B, h_kv, R, T, KEY_TILE)
    mt = St.amax(-1)
    vt = v.view(B, h_kv, T, KEY_TILE, d)
    out = []
    for num_splits in counts:
        if num_splits == 1:
            out += list(P.emulate(Q, K, V, keep, dtype))
            continue
        ns = min(num_splits, T)                                      # (splits past ceil(S_k / 64) are empty whatever the lengths)
        sid = torch.zeros(B, T, dtype=torch.long, device=dev)        # the split of each 64-key tile
        for b, n in enumerate(n_k):
            ch = split_chunk(n, num_splits)
            if ch:
                sid[b] = (torch.arange(T, device=dev) * KEY_TILE // ch).clamp(max=ns - 1)   # (tiles past N_k hold no visible key)
        idx = sid.view(B, 1, 1, T).expand(B, h_kv, R, T)
        ms = torch.full((B, h_kv, R, ns), -math.inf, dtype=f, device=dev).scatter_reduce(-1, idx, mt, "amax")
        m_use = torch.where(torch.isinf(ms), torch.zeros_like(ms), ms)
        Pt = torch.exp2(St - m_use.gather(-1, idx).unsqueeze(-1))
        Pr = Pt.to(dtype).to(f) if dtype in (torch.float16, torch.bfloat16) else Pt
        ot = torch.matmul(Pr.transpose(2, 3), vt).transpose(2, 3)                                   # (B, H_kv, R, T, d)
        l_s = torch.zeros(B, h_kv, R, ns, dtype=f, device=dev).scatter_add(-1, idx, Pt.sum(-1))
        o_s = torch.zeros(B, h_kv, R, ns, d, dtype=f, device=dev).scatter_add(-2, idx.unsqueeze(-1).expand(B, h_kv, R, T, d), ot)
        vis = l_s > 0
        one = torch.ones_like(l_s)
        O_s = (o_s * torch.where(vis, 1.0 / torch.where(vis, l_s, one), 0.0).unsqueeze(-1)).float()
        L_s = torch.where(vis, ms + torch.log2(torch.where(vis, l_s, one)), -math.inf).float()
        # fa2_decode_combine.hip
        m = L_s.amax(-1, keepdim=True)
        seen = ~torch.isinf(m)
        w = torch.where(seen, torch.exp2(L_s - torch.where(seen, m, torch.zeros_like(m))), 0.0)
        wsum = w.sum(-1, keepdim=True)
        inv = torch.where(seen, 1.0 / torch.where(seen, wsum, torch.ones_like(wsum)), 0.0)
        O = (w.unsqueeze(-1) * O_s).sum(-2) * inv
        L = torch.where(seen, m + torch.log2(torch.where(seen, wsum, torch.ones_like(wsum))), math.inf)
        out += [O.to(dtype), L.to(dtype)]
    return tuple(out)


def violations(O, L, O_ref, L_ref, dtype, split):
    """fa2_mask_probe.violations; float32 / float64 I/O through fp32 partials (split: the resolved num_splits > 1) is held to
    SPLIT_FP32_ULPS fp32 ulps of the truth instead of 4 ulps / 1e-6"""
    wide = split and dtype in (torch.float32, torch.float64)
    return P.violations(O, L, O_ref, L_ref, dtype, fp32_ulps=SPLIT_FP32_ULPS if wide else None)


def violated(O, L, O_ref, L_ref, dtype, split):
    """violations() of each sequence on its own -> bool (B,)"""
    wide = split and dtype in (torch.float32, torch.float64)
    return P.violated(O, L, O_ref, L_ref, dtype, fp32_ulps=SPLIT_FP32_ULPS if wide else None)


def fp32_ulp_error(O, L, O_ref, L_ref):
    """the largest |O - O_ref| and |L - L_ref| in fp32 ulps of the truth, over the rows that see a key"""
    fin = ~torch.isinf(L_ref)
    eo = ((O.double() - O_ref).abs() / ulp(O_ref, torch.float32))[fin.expand_as(O_ref)]
    el = ((L.double().reshape(L_ref.shape) - L_ref).abs() / ulp(L_ref, torch.float32))[fin]
    return (eo.max().item() if eo.numel() else 0.0), (el.max().item() if el.numel() else 0.0)


def measure_split_error(auto_splits=None):
    """-> (O, L, bad): the worst fp32-ulp error of emulate_split against the fp64 truth over the f32 / f64 grid of the GPU test at
    every split count > 1 -- the reference's own error, which SPLIT_FP32_ULPS is derived from -- and the bars the emulation breaks
    at any split count of the grid (auto_splits(g, N_q, d, dtype): what num_splits = 0 resolves to)"""
    worst_o = worst_l = 0.0
    bad = []
    for d in (64, 40):
        K, V = probe_cache(d)
        for g, n_q, causal, window in CONFIGS + VALU_CONFIGS:
            keep = decode_keep(g, n_q, causal, window)
            for uniform in (False, True):
                Q = probe_queries(g, n_q, d, uniform)
                for dtype in (torch.float32, torch.float64):
                    O_ref, L_ref = truth(Q, K, V, keep, dtype)
                    counts = sorted(set(SPLITS[1:]) | ({auto_splits(g, n_q, d, dtype)} if auto_splits else set()))
                    for n, (O, L) in emulate_splits(Q, K, V, keep, LENS, tuple(counts), dtype).items():
                        v = violations(O, L, O_ref, L_ref, dtype, n > 1)
                        if v:
                            bad.append(((g, n_q, causal, window), uniform, d, str(dtype), n, v))
                        if n > 1:
                            eo, el = fp32_ulp_error(O, L, O_ref, L_ref)
                            worst_o, worst_l = max(worst_o, eo), max(worst_l, el)
    return worst_o, worst_l, bad
