"""Exact-arithmetic probe for sparse MLA decode of packed (ragged) queries (fa2_fwd_kvcache_mla_sparse_varlen: the SP + VQ form of
fa2_decode_mla16.hip, the packed form of fa2_decode_sparse_generic.hip, the packed walk of fa2_decode_combine.hip, and the row-to-sequence
search fa2_varlen_owner they share with the packed selection).  TEST INFRASTRUCTURE ONLY: tests/test_decode_mla_sparse_varlen_probe.py
proves on the CPU that its bars see every planted error, tests/test_decode_mla_sparse_varlen_probe_gpu.py runs it through the Python
surface.  Device-agnostic.

It is tests/mla_sparse_probe.py (and through it tests/mla_probe.py and oracle/fa2_decode_probe.py) on a ragged batch, reused by import:
the latent rows, the one-hot queries, the value code, the fp64 truth, the fp32 restatement over the slots of a list, the entries that
are no key and the bars are theirs; no arithmetic and no bar is added.  What is new is the batch, the layout and the plants:

  * sequence b has N_Q[b] query tokens over N_K[b] keys, B = 11, total_q = 33, S_k = 2560: a leading empty sequence, two empty
    sequences in a row, a trailing one, a B that takes the owner search four steps deep, a token whose sequence has no key, three
    tokens over two keys, one sequence at full capacity, all lengths different;
  * the cache of (sequence b, KV head h) is latent row set u = b H_kv + h of mla_probe.latent_cache (mla_varlen_probe.cache's rule);
  * the queries of token i of sequence b are the rows r = head * n_q(b) + i of mla_probe.queries(g, n_q(b)), the same for each KV head;
  * lists(H_kv, topk) is int32 (total_q, H_kv, topk): per (packed row, KV head) distinct valid positions of the row's OWN sequence from a
    seeded permutation, mixed with -1, N_k(b), S_k + 5, 2^31 - 1 and -2^31; list (EMPTY_T, 0) has no valid entry although its sequence
    has keys, and where topk > 64 list (LATE_T, 0) has all its valid entries behind slot 64;
  * every (packed row t, KV head hk) is a pseudo-sequence p = t H_kv + hk of topk gathered rows under emulate_split, exactly as
    mla_sparse_probe.restate does it: gathered tensors are (total_q H_kv, 1, g, ...), to_call() brings O and L to the call's
    (total_q, H, 512) and (H, total_q), head = hk g + hg.

planted_outputs() hands one error each to the truth or to the restatement, modelled on the kernel's own expressions:

  owner_next / owner_prev        N_k and the cache rows (with them the descale and the table row) of sequence b + 1 / b - 1, cyclically
  owner_first_of_equal_offsets   the owner of a row behind a run of empty sequences taken as the first b of the run (equal offsets)
  list_by_position               the list of packed row t - start: the fixed kernel's position inside the sequence
  list_next_row                  the list of packed row t + 1
  q_by_position                  Q read at packed row t - start
  kv_head_0_list                 the list of KV head 0 for every KV head (hk * is[1] dropped)
  kv_head_other_cache            the cache rows of the other KV head
  partials_head_major            the combine reads partial row head * total_q + t where the kernel wrote t * H + head
  l_transposed                   L written as (total_q, H)
  off_by_one, invalid_as_key_0, decoy_accepted, past_topk_read, drop_last_partial, boundary_twice, boundary_skipped, wrong_page_size,
  physical_row                   mla_sparse_probe's, per list

Bars: oracle/fa2_decode_probe.violations unchanged.  The restatement's worst float32 error over this file's whole grid (every
configuration, both probes, every split count of SPLITS and what num_splits = 0 resolves to), measured by
tests/test_decode_mla_sparse_varlen_probe.py with oracle/fa2_decode_probe.fp32_ulp_error: 10.18 fp32 ulps on O and 1.22 on L
(MEASURED_FP32_ULPS, rounded up to 10.2) -- inside the oracle's SPLIT_MEASURED (12.8), so the float32 split bar SPLIT_FP32_ULPS (64)
stands as it is."""
import functools

import torch

import mla_probe as M
import mla_sparse_probe as S
from mla_probe import latent_cache, mla_truth, queries, restate, value_of  # noqa: F401 (the probe's own)
from mla_sparse_probe import NO_KEY, PAGE, SPLITS, WRONG_PAGE  # noqa: F401
from oracle.fa2_decode_probe import fp32_ulp_error, split_chunk, violated, violations  # noqa: F401

S_K = 2560
N_Q = [0, 1, 3, 0, 0, 2, 5, 1, 17, 4, 0]
N_K = [100, 0, 2, 64, 7, 65, 64, S_K, 1000, 300, 50]
B, TOTAL, MAX_Q = len(N_Q), sum(N_Q), max(N_Q)
CU = [0] + torch.tensor(N_Q).cumsum(0).tolist()
OWNER = [b for b, n in enumerate(N_Q) for _ in range(n)]          # the sequence of packed row t
POS = [i for n in N_Q for i in range(n)]                           # ... and its position t - start in it
NO_KEYS_B = N_K.index(0)                                           # the sequence without a key: its rows are decoys
EMPTY_T, LATE_T = CU[6], CU[8]  # a list without a valid entry (N_k 64); a list whose valid entries all sit behind slot 64 (N_k 1000)
# (H, H_kv, topk): a quarter, a partial, one and two head tiles (g = H / H_kv heads a list); every topk of the grid; two KV heads
CONFIGS = [(16, 1, 1), (40, 1, 63), (64, 1, 64), (128, 1, 65), (32, 2, 200), (128, 1, 2048), (40, 1, 2048), (256, 2, 200)]
MEASURED_FP32_ULPS = 10.2        # on O (10.18); 1.22 on L (the module docstring; re-measured and printed by the CPU proof)
LAYOUT_PLANTS = ("owner_next", "owner_prev", "owner_first_of_equal_offsets", "list_by_position", "list_next_row", "q_by_position",
                 "kv_head_0_list", "kv_head_other_cache", "partials_head_major", "l_transposed")
LIST_PLANTS = ("off_by_one", "invalid_as_key_0", "decoy_accepted", "past_topk_read", "drop_last_partial", "boundary_twice",
               "boundary_skipped", "wrong_page_size", "physical_row")
PLANTS = LAYOUT_PLANTS + LIST_PLANTS
OUTPUT_PLANTS = ("partials_head_major", "l_transposed")            # these only move finished rows


def cases(rotation=0):
    """(H, H_kv, topk, num_splits): every configuration under one split count, rotating with `rotation`"""
    return [cfg + (SPLITS[(k + rotation) % len(SPLITS)],) for k, cfg in enumerate(CONFIGS)]


@functools.lru_cache(maxsize=None)
def cache(h_kv=1, device=None):
    """the latent rows (B, H_kv, S_k, 576) in float64, decoys behind N_K[b]: (sequence b, KV head h) is row set u = b H_kv + h"""
    return latent_cache(lens=[n for n in N_K for _ in range(h_kv)], s_k=S_K, device=device).view(B, h_kv, S_K, M.D_QK)


def lists(h_kv, topk, device=None):
    """int32 (total_q, H_kv, topk), contiguous"""
    g = torch.Generator().manual_seed(1000 * h_kv + topk)
    idx = torch.empty(TOTAL, h_kv, topk, dtype=torch.int64)
    for t, b in enumerate(OWNER):
        nk = N_K[b]
        bad = torch.tensor(NO_KEY(nk))
        for hk in range(h_kv):
            perm = torch.randperm(max(nk, 1), generator=g)[:topk]
            row = bad[torch.randint(0, len(bad), (topk,), generator=g)]          # every slot no key ...
            take = torch.rand(topk, generator=g) < 0.8                            # ... but four in five, while positions last
            take &= torch.cumsum(take, 0) <= (perm.numel() if nk else 0)
            if hk == 0 and t == EMPTY_T:
                take[:] = False
            if hk == 0 and t == LATE_T and topk > 64:
                take[:64] = False
            row[take] = perm[:int(take.sum())]
            idx[t, hk] = row
    return idx.to(torch.int32).to(device)


def valid(idx):
    """(total_q, H_kv, topk) bool: the slots that are keys of the row's own sequence (mla_sparse_probe.valid, the rows as its batch)"""
    return S.valid(idx.unsqueeze(1), [N_K[b] for b in OWNER]).squeeze(1)


def packed_queries(g, h_kv, uniform=False, device=None):
    """Q (total_q, H, 576) in float64: token i of sequence b holds the rows r = head * n_q(b) + i of mla_probe.queries(g, n_q(b)),
    the same for each KV head"""
    per = []
    for n in N_Q:
        if n:
            q = queries(g, n, uniform, B=1, device=device)[0, 0].view(g, n, M.D_QK).transpose(0, 1)      # (n, g, 576)
            per.append(q.unsqueeze(1).expand(n, h_kv, g, M.D_QK).reshape(n, h_kv * g, M.D_QK))
    return torch.cat(per)


def to_call(O, L, h_kv):
    """(total_q H_kv, 1, g, ...) -> O (total_q, H, 512) and L (H, total_q) as the call returns them"""
    g = O.shape[2]
    return O.reshape(TOTAL, h_kv * g, O.shape[-1]), L.reshape(TOTAL, h_kv * g).t().contiguous()


def from_call(O, L, h_kv):
    """the call's O (total_q, H, 512), L (H, total_q) -> (total_q H_kv, 1, g, ...)"""
    g = O.shape[1] // h_kv
    return O.reshape(TOTAL * h_kv, 1, g, O.shape[-1]), L.t().reshape(TOTAL * h_kv, 1, g, 1)


def truth(Q, K, keep, dtype):
    """fp64 O (total_q H_kv, 1, g, 512), L (total_q H_kv, 1, g, 1)"""
    return S.truth(Q, K, keep, dtype)


def restate_slots(Q, K, keep, num_splits, dtype):
    """mla_sparse_probe.restate: emulate_split over the slots -> O, L in the I/O dtype"""
    return S.restate(Q, K, keep, num_splits, dtype)


def first_of_equal_offsets(b):
    """the first sequence whose offset equals sequence b's: b itself unless empty sequences stand in front of it"""
    return CU.index(CU[b])


def operands(g, h_kv, topk, uniform=False, plant=None, num_splits=3, device=None):
    """(Q (P, 1, g, 576), K (P, 1, T, 576), keep (P, 1, g, T)), P = total_q H_kv: what the restatement reads for every (packed row,
    KV head) under the planted input error `plant` (None: no error), or None where the plant cannot apply to this configuration"""
    if plant in OUTPUT_PLANTS:
        plant = None
    if plant in ("kv_head_0_list", "kv_head_other_cache") and h_kv < 2:
        return None
    ten = lambda x: torch.tensor(x, device=device)
    idx = lists(h_kv, topk, device).long()
    P = TOTAL * h_kv
    t, hk = torch.arange(P, device=device) // h_kv, torch.arange(P, device=device) % h_kv
    own, pos = ten(OWNER)[t], ten(POS)[t]
    own_c, hk_c, t_l, hk_l, t_q = own, hk, t, hk, t
    if plant == "owner_next":
        own_c = (own + 1) % B
    elif plant == "owner_prev":
        own_c = (own - 1) % B
    elif plant == "owner_first_of_equal_offsets":
        own_c = ten([first_of_equal_offsets(b) for b in range(B)])[own]
    elif plant == "list_by_position":
        t_l = pos
    elif plant == "list_next_row":
        t_l = (t + 1) % TOTAL
    elif plant == "q_by_position":
        t_q = pos
    elif plant == "kv_head_0_list":
        hk_l = torch.zeros_like(hk)
    elif plant == "kv_head_other_cache":
        hk_c = (hk + 1) % h_kv
    Q = packed_queries(g, h_kv, uniform, device).view(TOTAL, h_kv, g, M.D_QK)[t_q, hk].unsqueeze(1)
    e = idx[t_l, hk_l]                                                            # (P, T): the entries every slot reads
    nk = ten(N_K)[own_c].view(P, 1)
    keep = (e >= 0) & (e < nk)
    src = e
    rows = cache(h_kv, device).view(1, B * h_kv * S_K, M.D_QK)
    base = ((own_c * h_kv + hk_c) * S_K).view(P, 1)
    if plant == "off_by_one":
        src = (e + 1).clamp(max=S_K - 1)
    elif plant == "invalid_as_key_0":
        src, keep = torch.where(keep, e, torch.zeros_like(e)), torch.ones_like(keep)
    elif plant == "decoy_accepted":
        keep = keep | ((e == nk) & (e < S_K))
    elif plant == "past_topk_read":
        extra = -topk % 64
        if not extra:
            return None
        flat = torch.cat([idx.reshape(-1), torch.zeros(extra, dtype=idx.dtype, device=device)])   # (the last list's: 0)
        src = flat[(torch.arange(P, device=device) * topk).view(-1, 1) + torch.arange(topk + extra, device=device)]
        keep = (src >= 0) & (src < nk)
    elif plant == "drop_last_partial":
        if not topk % 64:
            return None
        keep = keep.clone()
        keep[:, topk - topk % 64:] = False
    elif plant in ("boundary_twice", "boundary_skipped"):
        c = split_chunk(topk, num_splits)
        if c >= topk:
            return None
        if plant == "boundary_skipped":
            keep = keep.clone()
            keep[:, c] = False
        else:
            src, keep = torch.cat([e, e[:, c:c + 1]], -1), torch.cat([keep, keep[:, c:c + 1]], -1)
    elif plant in ("wrong_page_size", "physical_row"):
        pl, table = S.pool(cache(h_kv, device), decoy=NO_KEYS_B)                  # (num_blocks, H_kv, PAGE, 576), (B, max_blocks)
        rows = pl.view(1, -1, M.D_QK)
        j = torch.where(keep, e, torch.zeros_like(e))
        if plant == "physical_row":
            src, base = j, torch.zeros_like(base)
        else:
            page = torch.gather(table.long()[own_c], 1, j // PAGE)
            src = ((page * h_kv + hk_c.view(P, 1)) * PAGE + j % WRONG_PAGE).clamp(max=rows.shape[1] - 1)
            base = torch.zeros_like(base)
    safe = torch.where(keep, src, torch.zeros_like(src))
    K, kp = S.gather(rows, (base + safe).view(1, 1, P, -1), torch.ones_like(keep).view(1, 1, P, -1), g)
    return Q, K, keep.view(P, 1, 1, -1).expand(-1, -1, g, -1)


def moved(name, O, L, h_kv):
    """finished (O, L) in the gathered layout under an output plant: the rows a combine or an L store with the wrong row expression
    hands back"""
    Oc, Lc = to_call(O, L, h_kv)
    H = Oc.shape[1]
    if name == "partials_head_major":           # row t * H + head answered with what was written at row head * total_q + t
        f = torch.arange(H, device=O.device).view(1, H) * TOTAL + torch.arange(TOTAL, device=O.device).view(TOTAL, 1)
        Oc = Oc.reshape(TOTAL * H, -1)[f]
        Lc = Lc.t().reshape(TOTAL * H)[f].t()
    elif name == "l_transposed":                # L[head, t] holds what was written at flat head * total_q + t of a (total_q, H) buffer
        Lc = Lc.t().reshape(H, TOTAL)
    else:
        raise ValueError(name)
    return from_call(Oc, Lc.contiguous(), h_kv)


def planted_outputs(name, fn, g, h_kv, topk, uniform=False, num_splits=3, device=None):
    """(O, L) of fn(Q, K, keep) -- the truth or the restatement, (total_q H_kv, 1, g, ...) -- under the plant `name` (None: no error),
    or None where it cannot apply"""
    got = operands(g, h_kv, topk, uniform, name, num_splits, device)
    if got is None:
        return None
    O, L = fn(*got)
    return moved(name, O, L, h_kv) if name in OUTPUT_PLANTS else (O, L)
