"""Exact-arithmetic probe for the packed forward with a value head size of its own (fa2_fwd_varlen_dv: d = 192, d_v = 128), in the
manner of tests/mla_probe.py.  TEST INFRASTRUCTURE ONLY: tests/test_mla_prefill_probe.py proves on the CPU that its bars see every
planted error, tests/test_mla_prefill_probe_gpu.py runs it through the Python surface.

The arithmetic is the mask probe's (oracle/fa2_mask_probe.py, whose truth, restatement, bars and masks are imported): scale =
fp32(ln 2), so c = scale * log2 e is exactly 1 in fp32; every score is an integer in [0, 8]; P is a power of two, exact in f16 and
bf16; l and P V are exact fp32 sums.  What this layout adds:

  * K (total_k, H_kv, 192): one score column in each of the 12 k-steps of a 32x32x16 MFMA, SCORE_COLS[k] = 16 k + (7 k mod 16) --
    eight below column 128 (the "nope" image) and four in 128..191 (the rotary image) -- holding (j (k + 1) + u) mod 5 for the
    packed key j of KV head u, the rest 0.
  * Q (total_q, H, 192): packed row i of head h has a 1 in one nope step, (i + h) mod 8, and in one rotary step,
    8 + (i + i // 32 + h) mod 4: every row's score has a contribution from both images, neighbouring rows (and rows r, r + 32)
    differ, and every k-step is some row's.  uniform=True: Q = 0, every visible key has weight 1, O is a count ratio and L = log2(count).
  * V (total_k, H_kv, 128): the mask probe's two-level one-hot of the key g = j + 17 u over 128 columns -- column g mod 64 and
    column 64 + (g // 64) mod 64 -- so an output column names the key and the column it came from: a V read 64 columns or one row
    stride off lands in columns that should be exactly 0.
"""
import torch

from oracle import fa2_mask_probe as P
from oracle.fa2_mask_probe import SCALE, emulate, heads_first, truth, violations  # noqa: F401  (re-exported)

D, D_V = 192, 128
KSTEPS = D // 16
SCORE_COLS = tuple(16 * k + (7 * k) % 16 for k in range(KSTEPS))
LQ = [0, 1, 31, 127, 128, 129, 300, 40]
LK = [5, 1, 65, 31, 128, 257, 300, 0]          # N_q < N_k, N_q > N_k, N_k = 0, N_q = 0
H = 4
H_KVS = (4, 2, 1)
WINDOWS = (None, (64, 0), (100, 50), (-1, 17))
PLANTS = ("no_rope_columns", "drop_kstep_5", "drop_kstep_10", "k_images_exchanged", "v_at_k_row_stride", "v_from_column_64",
          "o_at_stride_d", "right_plus_one", "left_minus_one", "top_left", "drop_last_partial_unit", "plus32", "kv_head_mod")


def cases():
    """(H_kv, causal, window): the grid of both test files"""
    return [(hk, causal, w) for hk in H_KVS for causal in (False, True) for w in WINDOWS]


def inputs(h_kv, uniform=False, device=None, lq=LQ, lk=LK):
    """Q (total_q, H, 192), K (total_k, H_kv, 192), V (total_k, H_kv, 128) in float64, every value exact in f16 and bf16"""
    tq, tk = sum(lq), sum(lk)
    Q = torch.zeros(tq, H, D, dtype=torch.float64, device=device)
    K = torch.zeros(tk, h_kv, D, dtype=torch.float64, device=device)
    V = torch.zeros(tk, h_kv, D_V, dtype=torch.float64, device=device)
    cols = torch.tensor(SCORE_COLS, device=device)
    i, j = torch.arange(tq, device=device), torch.arange(tk, device=device)
    for h in range(H):
        if not uniform:
            Q[i, h, cols[(i + h) % 8]] = 1.0
            Q[i, h, cols[8 + (i + i // 32 + h) % 4]] = 1.0
    for u in range(h_kv):
        for k in range(KSTEPS):
            K[:, u, SCORE_COLS[k]] = ((j * (k + 1) + u) % 5).double()
        V[:, u] = P.probe_qkv(0, tk, D_V, u, device=device)[2]
    return Q, K, V


def expand(t, h_kv, mod=False):
    """(total_k, H_kv, .) as (total_k, H, .): query head h reads KV head h // g (mod=True, the planted error: h % H_kv)"""
    idx = torch.arange(H, device=t.device)
    return t[:, idx % h_kv if mod else idx // (H // h_kv)]


def keep_of(causal, window, plant=None, device=None, lq=LQ, lk=LK):
    return P.varlen_keep(lq, lk, causal, window, plant=plant, device=device)


def reference(Q, K, V, h_kv, keep, dtype, fn=truth):
    """fn (truth or emulate) of the packed probe -> O (total_q, H, 128), L (H, total_q)"""
    q, k, v = heads_first(Q, expand(K, h_kv), expand(V, h_kv))
    O, L = fn(q, k, v, keep, dtype)
    return O.transpose(0, 1), L.squeeze(-1)


def _at_offset(V, h_kv, token_stride, head_stride, offset):
    """V's memory (contiguous (total_k, H_kv, 128), zeros behind it) read as (total_k, H_kv, 128) at other strides / another start"""
    tk = V.shape[0]
    flat = torch.cat([V.reshape(-1), torch.zeros(tk * h_kv * D + D, dtype=V.dtype, device=V.device)])
    j = torch.arange(tk, device=V.device).view(tk, 1, 1)
    u = torch.arange(h_kv, device=V.device).view(1, h_kv, 1)
    c = torch.arange(D_V, device=V.device).view(1, 1, D_V)
    return flat[j * token_stride + u * head_stride + c + offset]


def planted(name, Q, K, V, h_kv, causal, window, dtype, fn=truth, lq=LQ, lk=LK):
    """(O, L) of fn under the planted error `name` (PLANTS)"""
    dev = Q.device
    keep = keep_of(causal, window, device=dev, lq=lq, lk=lk)
    Ke, Ve = expand(K, h_kv), expand(V, h_kv)
    if name == "no_rope_columns":
        Ke = Ke.clone()
        Ke[..., 128:] = 0
    elif name.startswith("drop_kstep_"):
        k = int(name.rsplit("_", 1)[1])
        Ke = Ke.clone()
        Ke[..., 16 * k:16 * k + 16] = 0
    elif name == "k_images_exchanged":  # the rotary image read where the first 64 nope columns belong, and the reverse
        Ke = torch.cat([Ke[..., 128:192], Ke[..., 64:128], Ke[..., 0:64]], -1)
    elif name == "v_at_k_row_stride":
        Ve = expand(_at_offset(V, h_kv, h_kv * D, D, 0), h_kv)
    elif name == "v_from_column_64":
        Ve = expand(_at_offset(V, h_kv, h_kv * D_V, D_V, 64), h_kv)
    elif name in ("right_plus_one", "left_minus_one", "top_left"):
        keep = keep_of(causal, window, plant=name, device=dev, lq=lq, lk=lk)
    elif name == "drop_last_partial_unit":
        keep = keep.clone()
        k0 = 0
        for nk in lk:
            keep[:, k0 + (nk // 64) * 64:k0 + nk] = False
            k0 += nk
    elif name == "kv_head_mod":
        Ke, Ve = expand(K, h_kv, mod=True), expand(V, h_kv, mod=True)
    q, k, v = heads_first(Q, Ke, Ve)
    O, L = fn(q, k, v, keep, dtype)
    O, L = O.transpose(0, 1), L.squeeze(-1)
    if name == "o_at_stride_d":  # rows written 192 apart into O's memory, read back 128 apart; what is never written reads 0
        tq = O.shape[0]
        flat = torch.zeros(tq * H * D, dtype=O.dtype, device=dev)
        flat.view(tq * H, D)[:, :D_V] = O.reshape(tq * H, D_V)
        O = flat[:tq * H * D_V].view(tq, H, D_V)
    elif name == "plus32":  # rows r and r + 32 of a sequence exchanged (where both exist)
        idx = torch.arange(O.shape[0], device=dev)
        q0 = 0
        for nq in lq:
            r = torch.arange(nq, device=dev)
            s = r ^ 32
            idx[q0:q0 + nq] = q0 + torch.where(s < nq, s, r)
            q0 += nq
        O, L = O[idx], L[:, idx]
    return O, L


def sequences(lq=LQ):
    q0 = 0
    for nq in lq:
        yield slice(q0, q0 + nq)
        q0 += nq


def violations_of(O, L, O_ref, L_ref, dtype, rows=slice(None)):
    """oracle.fa2_mask_probe.violations of packed results (O (total_q, H, 128), L (H, total_q)) on the query rows `rows`"""
    return violations(O[rows].transpose(0, 1), L[:, rows].unsqueeze(-1), O_ref[rows].transpose(0, 1), L_ref[:, rows].unsqueeze(-1), dtype)
