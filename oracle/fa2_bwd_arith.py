"""The backward kernels' arithmetic, restated in float64 torch ops with the kernels' own rounding points.

TEST INFRASTRUCTURE ONLY (tests/test_bwd_arith.py pins it on the CPU, tests/test_bwd_elementwise.py compares the
kernels with it on the device).  Device-agnostic: it runs wherever its inputs live.

restate(Q, K, V, O, L, dO, causal, scale, kernel) takes the forward's own O and L exactly as stored (I/O dtype; O may be
a strided view) and returns dQ, dK, dV computed the way `kernel` computes them, plus element-wise bars (BwdArith.tol).
Everything is float64 except at the points where the kernel rounds; rnd() is RTNE to the I/O dtype (subnormals kept) by
torch's conversion, and the identity for float32 / float64 I/O (those kernels keep P and dS in their accumulator type).

The arithmetic (csrc/ = flash_attention_dlrs_amd/csrc/):
  c   = fp32(scale * log2 e), the product formed in double       fa2_bwd_mfma16.hip:801, fa2_bwd_mfma32.hip:339,
                                                                   fa2_bwd_generic.hip:414, :149 (float64 I/O: c stays double)
  D   = sum_x dO * O, O as stored                                   fa2_bwd_mfma16.hip:90-121, fa2_bwd_generic.hip:72-89
  S   = Q K^T;  P_u = exp2(c S - L), L as stored; 0 where masked   fa2_bwd_mfma16.hip:525 / :539, :567-576, generic :270-280
        (causal mask: key > query; rows and keys >= N: 0;
         window / varlen: outside band(), per sequence; a row with no visible key has L = +inf, so P = 0 and dQ = 0:
         fa2_bwd_mfma16.hip:673-675, fa2_bwd_generic.hip:318-324)
  tot = sum_j P_u                                                   fa2_bwd_mfma16.hip:577 / :644-650, generic :285-289
  Lc  = L + log2 tot  (the dQ launch hands it to the dK/dV launch)  fa2_bwd_mfma16.hip:678, generic :336
  dQ  = rnd(P_u (dP - D)) K * (scale / tot)       mfma16 / mfma32:  fa2_bwd_mfma16.hip:578, :593, :677
      = rnd(P_u (dP - D) scale) K / tot           generic:          fa2_bwd_generic.hip:282, :333
  P_n = exp2(c S - Lc), masked                                      fa2_bwd_mfma16.hip:454-463, generic :270-280
  dV  = rnd(P_n)^T dO                                               fa2_bwd_mfma16.hip:490 (dV waves), generic :295
  dK  = rnd(P_n (dP - D))^T Q * scale             mfma16 / mfma32:  fa2_bwd_mfma16.hip:482, :490, :681
      = rnd(P_n (dP - D) scale)^T Q               generic:          fa2_bwd_generic.hip:282, :296
  and the final RTNE cast of each gradient to the I/O dtype (fa2_bwd_mfma16.hip:667, generic E::store).
mfma32 is mfma16's arithmetic in fp32 (fa2_bwd_mfma32.hip:207-215, :270-274): rnd is the identity there.

What the restatement does NOT imitate (the kernels' liberties, covered by the bars below): every sum is exact here and
fp32 in the kernels, in the matrix pipe's order; exp2 is exact here and v_exp_f32 / exp2f (1 ulp) there; Lc is exact here
and fp32 there; c S - L is one fma in the MFMA kernels.

The bars (BwdArith.tol, one tensor per gradient; used by compare() below).  A gradient element
is a sum  g = m * sum_k t_k y_k  of terms t_k (rounded P or dS) times operands y_k (dO, Q, K), m the factor applied at the
store (scale, scale / tot, 1).  Kernel and restatement agree on the inputs; they differ by
  (1) the output rounding:                            one ulp of the I/O dtype at |g|;
  (2) one term t_k rounded to the other neighbour:    before its rounding, t_k differs from the restatement's by a relative
      ~1e-6 (below), which moves the RTNE result by one step of the I/O dtype when t_k sits that close to a rounding
      boundary (or on a tie): |m| * ulp(max_k |t_k|) * max_k |y_k|, one such flip per element (two in one sum need two terms
      within 1e-6 relative of a boundary: p ~ (2e-6 / 2^-8)^2 per pair);
  (3) everything of order fp32 u = 2^-24 in each term and in the sums (the many flips of small terms included: their
      expected total is the terms' relative error times their magnitude):  eps * |m| * sum_k |t_k|' |y_k|, where |t_k|'
      is |P| for P terms and P (sum_x |dO_x V_x| + sum_x |dO_x O_x|) for dS terms (what the round-off of the two dots
      dP and D, and so of dP - D, is relative to) and
          eps = 2^-24 * 16 * (sqrt(n) + sqrt(d) + E),  E = |c| max sum_x |Q_x K_x| + max |L| (log2 units).
      sqrt(n) and sqrt(d): fp32 sums of n terms and the d-term dots of S and dP (round-off grows like the square root of
      the term count for independent roundings, x 16 for the worst rows); E: an absolute error of the exponent c S - L is
      |c| sum |Q K| u (the fp32 S, the fma) + |L| u (the fp32 Lc), and P's relative error is ln 2 times it.
So tol = ulp_io(|g|) + (2) + (3).  Besides, compare() demands a minimum fraction of bit-identical elements, which is what
sees a rounding point moved: see its docstring.
"""
import math
from collections import namedtuple

import torch

KERNELS = ("mfma16", "mfma32", "generic")
# Errors the CPU tests plant in the restatement, to show that the bars catch them (tests/test_bwd_arith.py)
PLANTS = ("no_renorm", "drop_last_key", "diag_off_by_one", "ds_other_point", "scale_twice", "scale_none", "d_unrounded_o")
# ... and in the band of a window / varlen problem (band() below): one more key on the right or on the left of every row, the
# band aligned top-left instead of bottom-right
MASK_PLANTS = ("right_plus_one", "left_minus_one", "top_left")

BwdArith = namedtuple("BwdArith", "dQ dK dV tol noise")


def band(nq, nk, causal=False, window=None, device=None, plant=None):
    """(nq, nk) visible (query, key) pairs of a window / varlen problem, bottom-right aligned (include/fa2_fwd.h): query i
    sees key j iff i + (nk - nq) - left <= j <= i + (nk - nq) + right; a side of -1 is unbounded and causal clamps right to 0.
    plant (tests only): right_plus_one / left_minus_one move that edge out by one key (where it is bounded), shift_one moves
    both edges one key to the right, top_left drops the nk - nq shift."""
    left, right = (-1, -1) if window is None else window
    if causal:
        right = 0
    i = torch.arange(nq, device=device).view(nq, 1) + (0 if plant == "top_left" else nk - nq)
    j = torch.arange(nk, device=device).view(1, nk)
    dl = {"left_minus_one": 1, "shift_one": -1}.get(plant, 0)
    dr = {"right_plus_one": 1, "shift_one": 1}.get(plant, 0)
    keep = torch.ones(nq, nk, dtype=torch.bool, device=device)
    if left >= 0:
        keep &= j >= i - left - dl
    if right >= 0:
        keep &= j <= i + right + dr
    return keep


def c_log2e(scale, dtype):
    """c as the kernels form it: scale * log2 e in double, rounded to fp32 (double for float64 I/O)."""
    c = float(scale) * math.log2(math.e)
    return c if dtype == torch.float64 else float(torch.tensor(c, dtype=torch.float64).float())


def rnd(x, dtype):
    """RTNE to the I/O dtype (subnormals kept), back in x's dtype; the identity for fp32 / fp64 I/O."""
    return x.to(dtype).to(x.dtype) if dtype in (torch.float16, torch.bfloat16) else x


def ulp(x, dtype):
    """One unit in the last place of `dtype` at |x| (the subnormal step below the smallest normal)."""
    fi = torch.finfo(dtype)
    a = x.abs().clamp(min=fi.tiny)
    return torch.exp2(torch.floor(torch.log2(a))) * fi.eps


def restate(Q, K, V, O, L, dO, causal=False, scale=1.0, kernel="mfma16", plant=None, bars=True, acc=torch.float64, *,
            window=None, keep=None):
    """dQ, dK, dV (I/O dtype) of `kernel` for the problem, the element-wise bars and their term (3) alone (`noise`; float64,
    None if bars=False).
    Q, O, dO: (B, H, N_q, d), K, V: (B, H, N_k, d), in the I/O dtype, any strides; L: (B, H, N_q[, 1]) as the forward stored
    it.  The visible pairs: `keep` (N_q, N_k) if given, else band(N_q, N_k, causal, window) for a window or a rectangular
    problem, else all pairs or the causal tril.  A row without a visible key (L = +inf, as the varlen forward stores it)
    gets P = 0 and dQ = 0, as the kernels give it.
    `plant` puts one of PLANTS or MASK_PLANTS into the arithmetic (tests only); acc=torch.float32 runs the same arithmetic in
    fp32 (a valid implementation with the kernels' precision, which the bars must accept: tests/test_bwd_arith.py)."""
    assert kernel in KERNELS and (plant is None or plant in PLANTS or plant in MASK_PLANTS)
    io = Q.dtype
    f = acc
    B, H, N, d = Q.shape
    Nk = K.shape[2]
    q, k, v, o, do = (t.to(f) for t in (Q, K, V, O, dO))
    l = L.to(f).reshape(B, H, N, 1)
    c = c_log2e(scale, io)
    scale_at_store = kernel != "generic"
    if plant == "ds_other_point":
        scale_at_store = not scale_at_store

    S = torch.matmul(q, k.transpose(-1, -2))
    if keep is not None:
        assert plant not in MASK_PLANTS, "a mask plant needs the band, not an explicit keep"
        keep = keep.to(Q.device).clone()
    elif window is not None or Nk != N or plant in MASK_PLANTS:
        keep = band(N, Nk, causal, window, Q.device, plant if plant in MASK_PLANTS else None)
    else:
        keep = torch.ones(N, N, dtype=torch.bool, device=Q.device)
        if causal:
            keep = keep.tril(-1 if plant == "diag_off_by_one" else 0)
    if plant == "diag_off_by_one" and (window is not None or Nk != N):     # the band's own diagonal j = i + (Nk - N)
        keep &= ~torch.ones(N, Nk, dtype=torch.bool, device=Q.device).tril(Nk - N).triu(Nk - N)
    if plant == "drop_last_key":
        keep[..., Nk - 1] = False
    cS = (S * c).masked_fill(~keep, -math.inf)
    Pu = torch.exp2(cS - l)
    tot = Pu.sum(-1, keepdim=True)
    empty = torch.isinf(l)                             # no visible key: L = +inf stays, P = 0, dQ = 0
    Lc = l if plant == "no_renorm" else torch.where(empty, l, l + torch.log2(tot))
    Pn = torch.exp2(cS - Lc)
    if plant == "no_renorm":
        tot = torch.ones_like(tot)

    if plant == "d_unrounded_o":   # O before its rounding to the I/O dtype (exact softmax of the same scores)
        o = torch.matmul(torch.softmax(cS * math.log(2.0), dim=-1), v)
    D = (do * o).sum(-1, keepdim=True)
    dP = torch.matmul(do, v.transpose(-1, -2))
    s_in, s_out = (1.0, scale) if scale_at_store else (scale, 1.0)
    if plant == "scale_twice":
        s_out *= scale
    elif plant == "scale_none":
        s_in, s_out = 1.0, 1.0

    dSu = rnd(Pu * (dP - D) * s_in, io)
    dSn = rnd(Pn * (dP - D) * s_in, io)
    Pr = rnd(Pn, io)
    mq = (s_out / tot).masked_fill(empty, 0.0)         # dQ's factor at the store (per query row; 0 for an empty row)
    dQ = torch.matmul(dSu, k) * mq
    dK = torch.matmul(dSn.transpose(-1, -2), q) * s_out
    dV = torch.matmul(Pr.transpose(-1, -2), do)
    tol = noise = None
    if bars:
        absS = torch.matmul(q.abs(), k.abs().transpose(-1, -2)).masked_fill(~keep, 0)     # sum_x |q_x k_x|
        lf = l[~empty]                                 # (rows without a key carry L = +inf: no term of theirs)
        E = (abs(c) * absS.amax() + lf.abs().amax()).item() if lf.numel() else 0.0
        eps = 2.0 ** -24 * 16 * (math.sqrt(max(N, Nk)) + math.sqrt(d) + E)
        sq = abs(s_in)
        dots = torch.matmul(do.abs(), v.abs().transpose(-1, -2)) + (do * o).abs().sum(-1, keepdim=True)
        mag_dS_u = Pu * dots * sq                        # |t|' of the dS terms
        mag_dS_n = Pn * dots * sq
        ytop = lambda y: y.abs().amax(dim=-2, keepdim=True)     # max_k |y_k| per column
        # (2): one term rounded the other way -- ulp of the largest term of the sum times the largest operand
        flipQ = ulp(dSu.abs().amax(-1, keepdim=True), io) * ytop(k) * mq.abs()
        flipK = ulp(dSn.abs().amax(-2).unsqueeze(-1), io) * ytop(q) * abs(s_out)
        flipV = ulp(Pr.amax(-2).unsqueeze(-1), io) * ytop(do)
        if io not in (torch.float16, torch.bfloat16):
            flipQ = flipK = flipV = 0.0
        accQ = torch.matmul(mag_dS_u, k.abs()) * mq.abs()
        accK = torch.matmul(mag_dS_n.transpose(-1, -2), q.abs()) * abs(s_out)
        accV = torch.matmul(Pn.transpose(-1, -2), do.abs())
        noise = tuple(eps * a for a in (accQ, accK, accV))
        tol = tuple(ulp(g, io) + fl + n for g, fl, n in zip((dQ, dK, dV), (flipQ, flipK, flipV), noise))
    return BwdArith(dQ.to(io), dK.to(io), dV.to(io), tol, noise)


# Minimum fraction of bit-identical elements per gradient.  An element of the kernel's result differs from the restatement's
# when the two fp32 values before the final cast fall on different sides of an output rounding boundary: with the pre-cast
# difference of (2) + (3) above, a fraction ~ |difference| / ulp_io of the elements.  (3) is ~2^-24 * 16 * (sqrt(n) + ...)
# relative against ulp_io = 2^-8 (bf16) / 2^-11 (f16): a few percent of the elements at most, and a flip of (2) happens to
# one term in ~1e-6 / 2^-8 -- so 90 % is the floor for the 16-bit types.  It is counted over the elements whose output
# step is larger than their term (3): below it (a gradient that is a cancellation, |g| << sum |t y|, e.g. dQ of a row that
# sees one key, where dP - D = 0 up to fp32 round-off) the last bit is the summation order's.  A rounding point moved (dS rounded before
# instead of after the scale, D from another O) changes a large share of the terms of every sum by up to one step each
# and fails it.  fp32 / fp64 outputs are sums kept in their own precision: their last bits follow the summation order,
# so they are held to the element-wise bar only.
SAME_MIN = {torch.float16: 0.9, torch.bfloat16: 0.9, torch.float32: 0.0, torch.float64: 0.0}


def compare(got, ref, same_min=None):
    """[(name, fraction bit-identical, max |got - ref| / tol, ok)] for the three gradients: `got` (dQ, dK, dV) from a
    kernel, `ref` a BwdArith with bars.  ok: every element within its bar and at least `same_min` (default
    SAME_MIN[dtype]) of the elements bit-identical among those whose output ulp exceeds the bar's term (3)."""
    out = []
    for name, a, r, t, n in zip(("dQ", "dK", "dV"), got, ref[:3], ref.tol, ref.noise):
        assert a.shape == r.shape and a.dtype == r.dtype, (name, a.shape, r.shape, a.dtype, r.dtype)
        a = a.to(r.device)
        sm = SAME_MIN[r.dtype] if same_min is None else same_min
        sig = n < ulp(r.double(), r.dtype)
        same = (a == r)[sig].double().mean().item() if sig.any() else 1.0
        diff = (a.double() - r.double()).abs()
        worst = (diff / t).max().item() if a.numel() else 0.0
        finite = bool(torch.isfinite(a).all()) or not bool(torch.isfinite(r).all())
        out.append((name, same, worst, finite and worst <= 1.0 and same >= sm))
    return out


def assert_close(got, ref, what="", same_min=None):
    rep = compare(got, ref, same_min)
    assert all(ok for *_, ok in rep), (what, [(n, round(s, 4), round(w, 3)) for n, s, w, _ in rep])
    return rep
