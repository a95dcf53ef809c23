"""A torch restatement in fp64 of the MLA indexer (include/fa2_fwd.h, "The MLA indexer"): the candidate counts, the logits, the
rounding bar of the logits, and the selection exactly as it is stated -- sort by (value descending, position ascending), take the
prefix, sort by position, pad with -1.  No test of its own: tests/test_mla_indexer_*.py import it."""
import torch

F64 = torch.float64


def counts(lens, B, N_q, S_k, causal):
    """n(b, qi) as a list of lists: N_k(b) = clamp(lens[b]) (None: S_k), position p = N_k - N_q + qi; causal: min(p, N_k - 1) + 1
    keys, none for p < 0; else N_k"""
    out = []
    for b in range(B):
        nk = S_k if lens is None else min(max(int(lens[b]), 0), S_k)
        row = []
        for qi in range(N_q):
            p = nk - N_q + qi
            row.append(nk if not causal else (0 if p < 0 else min(p + 1, nk)))
        out.append(row)
    return out


def logits_f64(q, w, k, k_scale=None):
    """q (B, H, N_q, d), w (B, H, N_q), k (B, S_k, d) -- the STORED operands, an fp8 cache as its fp32 bytes' values --, k_scale
    (B, S_k) or None -> (B, N_q, S_k) fp64: k_scale[j] * sum_h w[h] * max(0, q[h] . k[j])"""
    out = torch.stack([(torch.einsum("hqd,kd->hqk", q[b].to(F64), k[b].to(F64)).clamp_(min=0) * w[b].to(F64)[..., None]).sum(0)
                       for b in range(q.shape[0])])  # (one sequence at a time: the (H, N_q, S_k) intermediate is the large one)
    return out if k_scale is None else out * k_scale.to(F64)[:, None, :]


def logits_bar(q, w, k, k_scale=None, terms=None):
    """The derived bar of an fp32 evaluation in any order: (d + H + 2) 2^-24 k_scale[j] sum_h |w[h]| sum_c |q[h, c] k[j, c]|, per
    element, in fp64"""
    B, H, N_q, d = q.shape
    out = torch.stack([(torch.einsum("hqd,kd->hqk", q[b].to(F64).abs(), k[b].to(F64).abs()) * w[b].to(F64).abs()[..., None]).sum(0)
                       for b in range(B)])
    if k_scale is not None:
        out = out * k_scale.to(F64)[:, None, :]
    return out * ((d + H + 2 if terms is None else terms) * 2.0 ** -24)


def select_row(values, topk):
    """one row of candidates (1-D, any float dtype) -> the list, a python list of topk ints"""
    v = values.detach().to(F64).cpu().clone()
    v[torch.isnan(v)] = -float("inf")  # a NaN ranks as -inf; -0.0 == +0.0 as numbers already
    order = torch.sort(-v, stable=True).indices  # value descending, ties in ascending position
    keep = sorted(order[:min(topk, v.numel())].tolist())
    return keep + [-1] * (topk - len(keep))


def topk_lists(logits, lens, topk, causal):
    """logits (B, N_q, S_k) -> int32 (B, N_q, topk) on the CPU; only entries j < n(b, qi) are looked at"""
    B, N_q, S_k = logits.shape
    n = counts(lens, B, N_q, S_k, causal)
    host = logits.detach().cpu()
    return torch.tensor([[select_row(host[b, qi, :n[b][qi]], topk) for qi in range(N_q)] for b in range(B)], dtype=torch.int32)


def candidate_mask(lens, B, N_q, S_k, causal, device="cpu"):
    """bool (B, N_q, S_k): j < n(b, qi)"""
    n = torch.tensor(counts(lens, B, N_q, S_k, causal), device=device)
    return torch.arange(S_k, device=device)[None, None, :] < n[..., None]


def paged(k, k_scale, page, seed, spare=3, fill=float("nan"), lens=None):
    """(pool, scale pool, block_table) of a contiguous cache k (B, S_k, d) and its scales (B, S_k) or None: the rows scattered over
    shuffled pages; `spare` pages that no table entry names and the rows of a last page past S_k hold decoy rows of `fill`.  With
    `lens`, the last table entry of the first sequence whose keys end before its last page is wild (2^30): no key lives there, and a
    kernel that looked it up all the same would be clamped into the pool."""
    B, S_k, d = k.shape
    mb = -(-S_k // page)
    g = torch.Generator().manual_seed(seed)
    nb = B * mb + spare
    table = torch.randperm(nb, generator=g)[:B * mb].to(torch.int32).view(B, mb)
    raw = lambda t: t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])  # (fp8 tensors are moved as bytes)
    pages = table.long().flatten().to(k.device)
    pool = torch.full((nb, page, d), fill, dtype=torch.float32, device=k.device).to(k.dtype)
    padded = torch.full((B, mb * page, d), fill, dtype=torch.float32, device=k.device).to(k.dtype)
    raw(padded)[:, :S_k] = raw(k)
    raw(pool)[pages] = raw(padded).view(B * mb, page, d)
    spool = None
    if k_scale is not None:
        spool = torch.full((nb, page), fill, dtype=torch.float32, device=k.device)
        spad = torch.full((B, mb * page), fill, dtype=torch.float32, device=k.device)
        spad[:, :S_k] = k_scale
        spool[pages] = spad.view(B * mb, page)
    if lens is not None:
        short = [b for b in range(B) if int(lens[b]) <= (mb - 1) * page]
        assert short, "no sequence leaves its last page unused"
        table[short[0], mb - 1] = 2 ** 30
    return pool, spool, table.to(k.device)
