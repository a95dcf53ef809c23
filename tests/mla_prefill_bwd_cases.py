"""What the tests of the packed backward with a value head size of its own (fa2_bwd_varlen_dv) share: the forward's length grid, the
data, a float64 forward that stores O and L as the kernels do, the fp64 autograd truth, and the per-sequence element-wise reference
built on oracle.fa2_bwd_arith.restate (imported, never copied: it takes a V of another width unchanged) -- with the errors the CPU
test plants into it (PLANTS).  Device-agnostic: everything runs where its inputs live."""
import functools
import math

import torch

from oracle import fa2_bwd_arith as A

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
# the forward's grid (tests/test_mla_prefill_gpu.py): every edge of the 128-row owned block, the 64-row swept tile and the 32-row wave
# block; N_q > N_k, N_q < N_k, an empty query side and an empty key side, in one batch
LQ = [0, 1, 31, 127, 128, 129, 300, 40]
LK = [5, 1, 65, 31, 128, 257, 300, 0]
H, D, DV = 4, 192, 128
SCALE = 1.0 / math.sqrt(192)
WINDOWS = (None, (64, 0), (100, 50), (-1, 17))
MASKS = [(causal, w) for causal in (False, True) for w in WINDOWS]
BWD_REL = {F16: 4e-3, BF16: 2.5e-2, F32: 2e-4, F64: 1e-6}      # the bars of tests/test_varlen_gpu.py


def starts(lengths):
    return [0] + torch.tensor(lengths).cumsum(0).tolist()


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def data(dtype, h_kv=H, d=D, d_v=DV, dist="normal", lq=tuple(LQ), lk=tuple(LK)):
    """Q, K, V, dO on the CPU.  normal: N(0, 1); onehot: every row of Q and K a signed unit vector times 6 (scores 0 or +-36 scale: rows
    of P with one dominant key and exact ties); latemax: N(0, 1) with the last key of every sequence 4 K-norms long, so that the row
    maximum arrives in the last swept tile."""
    g = torch.Generator().manual_seed(7000 + 10 * d + d_v + h_kv + len(dist))
    tq, tk = sum(lq), sum(lk)
    Q, K, V, dO = (torch.randn(n, h, c, generator=g) for n, h, c in ((tq, H, d), (tk, h_kv, d), (tk, h_kv, d_v), (tq, H, d_v)))
    if dist == "onehot":
        for t in (Q, K):
            idx = torch.randint(0, d, t.shape[:2], generator=g)
            sign = torch.randint(0, 2, t.shape[:2], generator=g) * 2.0 - 1.0
            t.zero_().scatter_(2, idx.unsqueeze(-1), (6.0 * sign).unsqueeze(-1))
    elif dist == "latemax":
        for e, n in zip(starts(lk)[1:], lk):
            if n:
                K[e - 1] *= 4.0
    else:
        assert dist == "normal"
    return tuple(t.to(dtype) for t in (Q, K, V, dO))


def per_sequence(lq, lk):
    cq, ck = starts(lq), starts(lk)
    return [(b, cq[b], lq[b], ck[b], lk[b]) for b in range(len(lq))]


def forward_stored(Q, K, V, lq, lk, causal, scale, window):
    """(O, L) as the forward stores them, from float64: O (total_q, H, d_v) and L (H, total_q) rounded to Q's dtype; a row without a
    visible key has O = 0 and L = +inf.  Differentiable in float64 up to the final cast (truth() uses it before the cast)."""
    O, L = forward_f64(Q.double(), K.double(), V.double(), lq, lk, causal, scale, window)
    return O.to(Q.dtype), L.to(Q.dtype)


def forward_f64(q, k, v, lq, lk, causal, scale, window):
    g = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)      # query head h reads KV head h // g
    outs, ls = [], []
    for _, q0, nq, k0, nk in per_sequence(lq, lk):
        S = torch.einsum("qhd,khd->hqk", q[q0:q0 + nq], k[k0:k0 + nk]) * f32(scale)
        m = A.band(nq, nk, causal, window, q.device)
        S = S.masked_fill(~m, -math.inf)
        vis = m.any(-1)
        P = torch.where(vis.view(1, nq, 1), torch.softmax(S.masked_fill(~vis.view(1, nq, 1), 0.0), -1), 0.0)
        outs.append(torch.einsum("hqk,khd->qhd", P, v[k0:k0 + nk]))
        ls.append(torch.where(vis, torch.logsumexp(S, -1) * math.log2(math.e), math.inf))
    return torch.cat(outs), torch.cat(ls, 1)


def truth(Q, K, V, dO, lq, lk, causal, scale, window, head_of=None):
    """fp64 autograd through the per-sequence masked softmax: (dQ, dK, dV) with K's and V's head counts (the group sum is autograd's).
    head_of (tests only): another map from query head to KV head, as a list."""
    q, k, v = (t.detach().double().clone().requires_grad_() for t in (Q, K, V))
    if head_of is None:
        O, _ = forward_f64(q, k, v, lq, lk, causal, scale, window)
    else:
        O, _ = forward_f64(q, k[:, head_of], v[:, head_of], lq, lk, causal, scale, window)
    O.backward(dO.double())
    return q.grad, k.grad, v.grad


def within_truth(got, ref, dtype, factor=1.0):
    """[(name, max error, bound)] of the gradients that miss the BWD_REL bar of tests/test_varlen_gpu.py"""
    out = []
    for name, a, b in zip(("dQ", "dK", "dV"), got, ref):
        err = (a.double() - b.to(a.device)).abs().max().item() if a.numel() else 0.0
        bound = factor * BWD_REL[dtype] * max(1.0, b.abs().max().item() if b.numel() else 0.0)
        if not err <= bound or bool(torch.isnan(a).any()):
            out.append((name, err, bound))
    return out


def seq(t, start, n):
    """tokens [start, start + n) of a packed (total, H, c) tensor as restate's (1, H, n, c)"""
    return t[start:start + n].transpose(0, 1).unsqueeze(0)


# Errors planted into the reference (tests/test_mla_prefill_bwd_arith.py): each is what one wrong kernel would compute.
PLANTS = ("no_rotary", "k_step_missing", "dk_images_exchanged", "v_at_k_stride", "d_over_192", "dv_at_stride_d", "right_plus_one",
          "left_minus_one", "top_left", "last_tile_dropped", "rows_32_exchanged")


def restate_seq(Q, K, V, O, L, dO, q0, nq, k0, nk, causal, scale, window, kernel, plant=None, bars=True, acc=torch.float64):
    """restate() of one sequence of a packed batch with H_kv == H: a BwdArith over (1, H, n, c) tensors."""
    d, d_v = Q.shape[2], V.shape[2]
    q, k, v, o, do = seq(Q, q0, nq), seq(K, k0, nk), seq(V, k0, nk), seq(O, q0, nq), seq(dO, q0, nq)
    keep = A.band(nq, nk, causal, window, Q.device, plant if plant in A.MASK_PLANTS else None)
    if plant == "last_tile_dropped":                         # the last partial 64-row swept tile of either launch
        keep[:, nk - nk % 64:] = False
        keep[nq - nq % 64:, :] = False
    qs, ks = q, k
    if plant == "no_rotary":                                 # the rotary columns 128..191 left out of the score
        qs = q.clone()
        qs[..., 128:] = 0
    elif plant == "k_step_missing":                          # one of the 12 k-steps (16 columns) left out
        qs = q.clone()
        qs[..., 144:160] = 0
    elif plant == "v_at_k_stride":                           # dP over 192 columns of a V read at K's row stride (V enters dP alone)
        flat = torch.cat([v.reshape(1, v.shape[1], -1), torch.zeros(1, v.shape[1], nk * (d - d_v) + d, dtype=v.dtype, device=v.device)], -1)
        v = torch.stack([flat[..., d * j:d * j + d_v] for j in range(nk)], 2)
    elif plant == "d_over_192":                              # D summed over 192 columns: 64 of the next row's (O enters D alone)
        nxt = (do.double() * o.double()).roll(-1, 2)[..., :d - d_v].sum(-1)
        o = o.double().clone()
        lead = do.double()[..., 0]
        o[..., 0] += torch.where(lead != 0, nxt / torch.where(lead != 0, lead, torch.ones_like(lead)), torch.zeros_like(nxt))
    ref = A.restate(qs, ks, v, o, L[:, q0:q0 + nq].unsqueeze(0), do, causal, scale, kernel, bars=bars, acc=acc, keep=keep)
    dQ, dK, dV = ref.dQ, ref.dK, ref.dV
    if plant == "dk_images_exchanged":                       # dK's columns 128..191 and 0..63 (the two LDS images)
        dK = torch.cat([dK[..., 128:], dK[..., 64:128], dK[..., :64]], -1)
    elif plant == "dv_at_stride_d":                          # dV written at row stride d into rows of d_v
        flat = torch.zeros(1, dV.shape[1], nk * d + d_v, dtype=dV.dtype, device=dV.device)
        for j in range(nk):
            flat[..., d * j:d * j + d_v] = dV[:, :, j]
        dV = flat[..., :nk * d_v].reshape(dV.shape)
    elif plant == "rows_32_exchanged" and nk >= 64:          # owned rows r and r + 32 of the first block
        dK = torch.cat([dK[:, :, 32:64], dK[:, :, :32], dK[:, :, 64:]], 2)
    return A.BwdArith(dQ, dK, dV, ref.tol, ref.noise)


def reference(Q, K, V, O, L, dO, lq, lk, causal, scale, window, kernel, plant=None, bars=True, acc=torch.float64):
    """{sequence: BwdArith} over the sequences with queries and keys (the others get zero gradients: check_empty)."""
    return {b: restate_seq(Q, K, V, O, L, dO, q0, nq, k0, nk, causal, scale, window, kernel, plant, bars, acc)
            for b, q0, nq, k0, nk in per_sequence(lq, lk) if nq and nk}


def split(grads, lq, lk):
    """{sequence: (dQ, dK, dV) as (1, H, n, c)} of packed gradients, and the list of what is not exactly 0 in a sequence without
    queries or without keys"""
    dQ, dK, dV = grads
    out, nonzero = {}, []
    for b, q0, nq, k0, nk in per_sequence(lq, lk):
        if nq and nk:
            out[b] = (seq(dQ, q0, nq), seq(dK, k0, nk), seq(dV, k0, nk))
        elif bool((dQ[q0:q0 + nq] != 0).any()) or bool((dK[k0:k0 + nk] != 0).any()) or bool((dV[k0:k0 + nk] != 0).any()):
            nonzero.append(b)
    return out, nonzero


def pack(ref, lq, lk, like):
    """packed (dQ, dK, dV) of a {sequence: BwdArith}, zeros where a sequence has no reference"""
    Q, K, V = like
    dQ, dK, dV = torch.zeros_like(Q), torch.zeros_like(K), torch.zeros_like(V)
    for b, q0, nq, k0, nk in per_sequence(lq, lk):
        if b in ref:
            dQ[q0:q0 + nq], dK[k0:k0 + nk], dV[k0:k0 + nk] = (t[0].transpose(0, 1) for t in ref[b][:3])
    return dQ, dK, dV
