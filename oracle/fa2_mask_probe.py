"""Exact-arithmetic mask probe for the windowed and variable-length forward kernels.

TEST INFRASTRUCTURE ONLY (tests/test_mask_probe.py proves on the CPU that its bars see every planted mask error;
tests/test_mask_probe_gpu.py runs it through every forward form that takes a window or a varlen layout).  Device-agnostic.

The inputs make every forward kernel's arithmetic exact, so the fp64 truth can be demanded to within one output rounding:
  * scale = fp32(ln 2): c = fp32(scale * log2 e) is exactly 1.0 (the product is 1 + 2.7e-9), so c S is S.  (float64 I/O keeps
    c = 1 + 2.7e-9 in double: the truth below uses the kernel's own c, and fp64 is held to the 1e-6 bar of the window tests.)
  * Q[i, 0] = 1 and K[j, 0] = (7 (j + 5 u) mod 9), the rest 0 (u: the head / batch index): every score is an integer in [0, 8].
    P = exp2(S - m) is then a power of two in [2^-8, 2^8] whatever running maximum the kernel defers to (its threshold is
    12 / 60 log2 units), exact in bf16, f16 and fp8, and l and P V are exact fp32 sums.
  * V is a two-level one-hot of the GLOBAL key index g (the packed token for varlen, plus 17 u): with w = d // 2, columns
    g mod w and w + (g // w) mod w are 1.  A key that leaks in lands in a column that should be exactly 0, or moves a count
    by at least 1 / (k + 1); a key of the neighbouring sequence shows up in its own column.
  * uniform=True: Q = 0, so every visible key has weight 1, O is a count ratio and L = log2(count).
What is left is O = o * (1 / l) in fp32 (two roundings), L = m + log2 l in fp32 (v_log_f32), and the cast to the I/O dtype.

Bars (violations()): |O - O_ref| <= ulp_io(|O_ref|); O_ref == 0 exactly -> O == 0 exactly; |L - L_ref| <= ulp_io(|L_ref|);
empty rows (varlen): O = 0 and L = +inf exactly.  float32 I/O: 4 fp32 ulps (the division's two roundings, exp2f and log2f at
1 ulp each, and c = 1 against the truth's 1 + 2.7e-9 ~ 0.2 ulp at |S| <= 8).  float64 I/O: 1e-6 absolute (O) and
1e-6 max(1, |L|) (L).
"""
import math
import random

import numpy as np
import torch

from oracle.fa2_bwd_arith import band, c_log2e, ulp

SCALE = float(np.float32(math.log(2.0)))

# the GPU grid (tests/test_mask_probe_gpu.py) and the CPU sensitivity proof (tests/test_mask_probe.py) walk the same cases
SIDES = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 191, 255, 256, 257, -1)
NS = (1, 31, 32, 33, 64, 65, 200, 256, 257, 1000, 2065)
PLANTS = ("right_plus_one", "left_minus_one", "shift_one", "top_left", "neighbour_row")
DENSE_PLANTS = PLANTS[:3]


def window_cases():
    """(N, window, causal): every left side with three right sides and every right side with three left sides, N and causal
    rotating deterministically through NS and both settings (causal only where the right side is the one varied: causal
    clamps it to 0)."""
    out = []
    n = len(SIDES)
    for a, s in enumerate(SIDES):
        for r in range(3):
            t = SIDES[(7 * a + 5 * r + 3) % n]
            k = 3 * a + r
            out.append((NS[k % len(NS)], (s, t), k % 4 == 3))
            out.append((NS[(k + 5) % len(NS)], (t, s), False))
    return sorted(set(out), key=out.index)


# varlen mixes: N_k - N_q of 0, +-1, +-31, +-33, +-63, +-65, +-127, +-129; empty sequences on either side; N_q = 1; lengths
# that straddle 32, 64, 128 and 256
VARLEN_MIXES = [
    ([1, 33, 64, 0, 129, 257], [1, 2, 95, 9, 0, 256]),                   # 0, -31, +31, empty q, empty k, -1
    ([31, 32, 65, 128, 1, 300], [64, 65, 0, 1, 130, 171]),               # +33, +33, empty k, -127, +129, -129
    ([200, 63, 127, 256, 0, 33], [137, 128, 62, 321, 0, 0]),             # -63, +65, -65, +65, (0, 0), empty k
    ([97, 1, 255, 129, 40], [226, 64, 256, 0, 7]),                       # +129, +63, +1, empty k, -33
    ([129, 64, 2, 257, 300], [129, 1, 131, 128, 300]),                   # 0, -63, +129, -129, 0
    ([5, 160, 96, 1, 1000], [6, 33, 127, 33, 1001]),                     # +1, -127, +31, +32, +1
]
VARLEN_WINDOWS = [(None, False), (None, True), ((0, 0), False), ((1, 0), True), ((15, 17), False), ((31, 33), False),
                  ((63, -1), False), ((-1, 64), False), ((65, 1), False), ((127, 129), False), ((256, -1), True),
                  ((-1, 0), False), ((16, 95), False), ((191, 32), True)]


# strided (B, N, H, d) views and the padded head sizes 40 and 96 (tests/test_mask_probe_gpu.py)
LAYOUT_CASES = [(300, (17, 0), True), (300, (40, 9), False), (257, (65, 1), False), (200, (-1, 33), False),
                (333, (128, -1), False)]


# the packed batch test_probe_strided_views_and_padded_head_sizes reads from a strided buffer, and its windows
LAYOUT_VARLEN = ([100, 257, 33, 0, 64], [100, 256, 66, 5, 1], [((17, 3), False), (None, True), ((64, -1), False)])


def fp8_applies(window, causal, d):
    """fp8 runs the probe on dense windows no wider than the one-hot width d / 2 (not on varlen: e4m3fn has no +inf for an
    empty row)"""
    if window is None:
        return False
    left, right = window
    right = 0 if causal else right
    return left >= 0 and right >= 0 and left + right + 1 <= d // 2


# the seeded sweep of tests/test_window_varlen_fuzz_gpu.py (here so that tests/test_mask_probe.py proves its probe cases too)
FUZZ_EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 191, 255, 256, 257, 383, 511, 513, 777, 1025]


def _fuzz_side(rng):
    return rng.choice([-1, rng.choice(SIDES), rng.randint(0, 300)])


def _fuzz_draw(rng):
    d = rng.choice([32, 64, 64, 128, 128])
    dtype = rng.choice([torch.bfloat16, torch.bfloat16, torch.float16, torch.float32])
    return d, dtype, (_fuzz_side(rng), _fuzz_side(rng)), rng.random() < 0.3, rng.choice([1.0, 0.3, 1 / math.sqrt(d)])


def fuzz_window_cases():
    """48 x (B, H, N, d, dtype, window, causal, scale)"""
    rng = random.Random(20261016)
    out = []
    for k in range(48):
        N = rng.choice(FUZZ_EDGES) if k % 3 else rng.randint(1, 1100)
        B, H = rng.choice([(1, 1), (1, 3), (2, 2), (1, 8), (3, 2)])
        out.append((B, H, N) + _fuzz_draw(rng))
    return out


def fuzz_varlen_cases():
    """48 x (lq, lk, H, d, dtype, window, causal, scale)"""
    rng = random.Random(20261017)
    out = []
    for k in range(48):
        lq = [rng.choice(FUZZ_EDGES[:21] + [0, rng.randint(0, 600)]) for _ in range(rng.randint(1, 5))]
        lk = [max(0, n + rng.choice([0, 0, 1, -1, 31, -31, 33, -33, 63, -63, 65, -65, 127, -127, 129, -129]))
              if rng.random() < 0.85 else rng.choice([0, rng.randint(0, 600)]) for n in lq]
        if not sum(lq):        # (some query and some key in every batch)
            lq[0] = 1
        if not sum(lk):
            lk[0] = 1
        out.append((lq, lk, rng.choice([1, 2, 3])) + _fuzz_draw(rng))
    return out


def varlen_cases():
    """(lq, lk, window, causal): every mix under a rotating share of the windows (every window under two mixes at least)."""
    out = []
    for m, (lq, lk) in enumerate(VARLEN_MIXES):
        for w in range(len(VARLEN_WINDOWS)):
            if (w + m) % 3 != 2:
                window, causal = VARLEN_WINDOWS[w]
                out.append((lq, lk, window, causal))
    return out


def _cu(lengths):
    return [0] + np.cumsum(lengths).tolist()


def dense_keep(N, causal, window, plant=None, device=None):
    """(N, N) visible pairs of a dense window problem (bottom-right = top-left for square problems)"""
    return band(N, N, causal, window, device, plant=plant)


def varlen_keep(lq, lk, causal, window, plant=None, device=None):
    """(total_q, total_k) visible pairs of a packed batch: block-diagonal over the sequences, bottom-right aligned inside
    each (fa2_varlen_band).  neighbour_row: the middle row of the first sequence that has a neighbour with keys takes its
    band (same row index relative to the end of the sequence) from that neighbour's block."""
    cq, ck = _cu(lq), _cu(lk)
    keep = torch.zeros(cq[-1], ck[-1], dtype=torch.bool, device=device)
    per = plant if plant in ("right_plus_one", "left_minus_one", "shift_one", "top_left") else None
    for b, (nq, nk) in enumerate(zip(lq, lk)):
        if nq and nk:
            keep[cq[b]:cq[b] + nq, ck[b]:ck[b] + nk] = band(nq, nk, causal, window, device, plant=per)
    if plant == "neighbour_row":
        for b, nq in enumerate(lq):
            for nb in (b + 1, b - 1):
                if nq and 0 <= nb < len(lq) and lq[nb] and lk[nb]:
                    i = nq // 2
                    other = band(lq[nb], lk[nb], causal, window, device)
                    rel = max(0, lq[nb] - (nq - i))       # the same distance from the sequence's last row
                    row = torch.zeros(ck[-1], dtype=torch.bool, device=device)
                    row[ck[nb]:ck[nb] + lk[nb]] = other[rel]
                    if not torch.equal(row, keep[cq[b] + i]):
                        keep[cq[b] + i] = row
                        return keep
    return keep


def probe_qkv(nq, nk, d, u=0, uniform=False, device=None):
    """Q (nq, d), K (nk, d), V (nk, d) in float64 for head / batch index u; key g of V is the global key index"""
    Q = torch.zeros(nq, d, dtype=torch.float64, device=device)
    K = torch.zeros(nk, d, dtype=torch.float64, device=device)
    V = torch.zeros(nk, d, dtype=torch.float64, device=device)
    if not uniform:
        Q[:, 0] = 1.0
    g = torch.arange(nk, device=device) + 17 * u
    K[:, 0] = ((7 * (g + 5 * u)) % 9).double()
    w = d // 2
    V[torch.arange(nk, device=device), g % w] = 1.0
    V[torch.arange(nk, device=device), w + (g // w) % w] += 1.0
    return Q, K, V


def dense_inputs(B, H, N, d, dtype, uniform=False, device=None):
    """(B, H, N, d) probe tensors in the I/O dtype (every value exact in it)"""
    ts = [torch.empty(B, H, N, d, dtype=torch.float64, device=device) for _ in range(3)]
    for b in range(B):
        for h in range(H):
            for t, x in zip(ts, probe_qkv(N, N, d, b * H + h, uniform, device)):
                t[b, h] = x
    return tuple(t.to(dtype) for t in ts)


def varlen_inputs(lq, lk, H, d, dtype, uniform=False, device=None):
    """packed (total_q, H, d), (total_k, H, d) probe tensors: the key index is the packed token index"""
    tq, tk = sum(lq), sum(lk)
    Q, K, V = (torch.empty(n, H, d, dtype=torch.float64, device=device) for n in (tq, tk, tk))
    for h in range(H):
        q, _, _ = probe_qkv(tq, 0, d, h, uniform, device)
        _, k, v = probe_qkv(0, tk, d, h, uniform, device)
        Q[:, h], K[:, h], V[:, h] = q, k, v
    return tuple(t.to(dtype) for t in (Q, K, V))


def truth(Q, K, V, keep, dtype, scale=SCALE):
    """fp64 O and L (log2 units) of (…, nq, d) inputs under `keep` (nq, nk), with the kernel's own c; rows without a visible key:
    O = 0, L = +inf"""
    c = c_log2e(scale, dtype)
    q, k, v = Q.double(), K.double(), V.double()
    S = torch.matmul(q, k.transpose(-1, -2)) * c
    S = S.masked_fill(~keep, -math.inf)
    vis = keep.any(-1, keepdim=True)
    m = torch.where(vis, S.amax(-1, keepdim=True), torch.zeros_like(S[..., :1]))
    P = torch.exp2(S - m)
    l = P.sum(-1, keepdim=True)
    O = torch.where(vis, torch.matmul(P, v) / torch.where(vis, l, torch.ones_like(l)), 0.0)
    L = torch.where(vis, m + torch.log2(l), math.inf)
    return O, L


def emulate(Q, K, V, keep, dtype, scale=SCALE):
    """a valid fp32 implementation: S, l and P V in fp32, P rounded to the I/O dtype before P V, O = o * (1 / l) and
    L = m + log2 l in fp32, then the cast to the I/O dtype (what the bars must accept)"""
    f = torch.float32 if dtype != torch.float64 else torch.float64
    c = c_log2e(scale, dtype)
    q, k, v = (t.to(f) for t in (Q, K, V))
    S = (torch.matmul(q, k.transpose(-1, -2)) * c).masked_fill(~keep, -math.inf)
    vis = keep.any(-1, keepdim=True)
    m = torch.where(vis, S.amax(-1, keepdim=True), torch.zeros_like(S[..., :1]))
    P = torch.exp2(S - m)
    Pr = P.to(dtype).to(f) if dtype not in (torch.float32, torch.float64) else P
    l = P.sum(-1, keepdim=True)
    inv = torch.where(vis, 1.0 / torch.where(vis, l, torch.ones_like(l)), 0.0)
    O = torch.matmul(Pr, v) * inv
    L = torch.where(vis, m + torch.log2(l), math.inf)
    return O.to(dtype), L.to(dtype)


def _ulp_io(x, dtype):
    return ulp(x, torch.float16 if dtype == torch.float16 else dtype)


def _bars(O, L, O_ref, L_ref, dtype, fp32_ulps=None):
    """the bars element by element -> (nan, misplaced +inf in L, nonzero O where the truth is 0, |O - O_ref| in bars,
    |L - L_ref| in bars); the last two are 0 on the empty rows"""
    O, L = O.double().to(O_ref.device), L.double().to(O_ref.device).reshape(L_ref.shape)
    empty = torch.isinf(L_ref)
    nan = torch.isnan(O).any(-1, keepdim=True) | torch.isnan(L)
    inf = (torch.isinf(L) & (L > 0)) != empty
    nonzero = ((O_ref == 0) | empty) & (O != 0)
    if fp32_ulps is not None and dtype in (torch.float32, torch.float64):
        tolO, tolL = fp32_ulps * ulp(O_ref, torch.float32), fp32_ulps * ulp(L_ref, torch.float32)
    elif dtype == torch.float64:
        tolO = torch.full_like(O_ref, 1e-6)
        tolL = 1e-6 * L_ref.abs().clamp(min=1)
    elif dtype == torch.float32:
        tolO, tolL = 4 * ulp(O_ref, dtype), 4 * ulp(L_ref, dtype)
    else:
        tolO, tolL = _ulp_io(O_ref, dtype), _ulp_io(L_ref, dtype)
    eo = torch.where(empty, 0.0, (O - O_ref).abs() / tolO)
    el = torch.where(empty, 0.0, (L - L_ref).abs() / tolL)
    return nan, inf, nonzero, eo, el


def violations(O, L, O_ref, L_ref, dtype, fp32_ulps=None):
    """list of the bars O, L break (empty: pass).  O, L in the I/O dtype, any device; O_ref (…, nq, d), L_ref (…, nq, 1).
    fp32_ulps (float32 / float64 I/O only): that many fp32 ulps of the truth instead of the bars above, for a result that went
    through fp32 partials (oracle/fa2_decode_probe.py); the exact-zero and the empty-row rules stay."""
    nan, inf, nonzero, eo, el = _bars(O, L, O_ref, L_ref, dtype, fp32_ulps)
    out = []
    if nan.any():
        out.append("nan")
    if inf.any():
        out.append("L = +inf exactly on the empty rows")
    if nonzero.any():
        out.append(f"O != 0 where O_ref == 0: {int(nonzero.sum())} elements")
    if eo.numel() and eo.max() > 1:
        out.append(f"|O - O_ref| up to {eo.max().item():.3g} bars ({int((eo > 1).sum())} elements)")
    if el.numel() and el.max() > 1:
        out.append(f"|L - L_ref| up to {el.max().item():.3g} bars ({int((el > 1).sum())} elements)")
    return out


def violated(O, L, O_ref, L_ref, dtype, fp32_ulps=None):
    """violations() of each slice along the first axis at once -> bool (n,): True where the slice breaks a bar"""
    n = O_ref.shape[0]
    return torch.stack([(t > 1 if t.dtype.is_floating_point else t).reshape(n, -1).any(-1)
                        for t in _bars(O, L, O_ref, L_ref, dtype, fp32_ulps)]).any(0)


def heads_first(*ts):
    """packed (total, H, d) tensors as (H, total, d) views: the layout truth(), emulate() and violations() take"""
    return tuple(t.transpose(0, 1) for t in ts)
