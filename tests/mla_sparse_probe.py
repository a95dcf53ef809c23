"""Exact-arithmetic probe for sparse MLA decode (fa2_fwd_kvcache_mla_sparse): tests/mla_probe.py -- the latent rows whose value code
names every key that reached the output, reused by import -- under per-query key lists.  TEST INFRASTRUCTURE ONLY:
tests/test_decode_mla_sparse_probe.py proves on the CPU that its bars see every planted error, tests/test_decode_mla_sparse_probe_gpu.py
runs it through the Python surface.  Device-agnostic.

One batch of LENS at capacity S_K, H_kv = 1.  lists(N_q, topk): for every (b, qi) distinct valid positions from a seeded permutation
of [0, N_k(b)), mixed with entries that are no key (-1, N_k(b), S_k + 5, 2^31 - 1, -2^31) at seeded slots; one list (sequence EMPTY_B,
position 0) has none, and where topk > 64 one (sequence LATE_B, position 0) has all its valid entries behind slot 64.

The restatement is oracle.fa2_decode_probe.emulate_split on the GATHERED rows: every (b, qi) is a pseudo-sequence of length topk whose
key s is the row its slot s names, with the slot's validity as `keep` -- so the split rule of the emulation, ceil(topk / num_splits)
rounded up to 64, is the split over slots.  A slot that is no key gathers row 0 of the sequence and is masked.  plant_*() apply one
error each to what the restatement gathers or keeps; the paged ones read through a pool of PAGE-row pages (pool()).

Layouts: gathered tensors are (B * N_q, 1, H, ...) with pseudo-sequence p = b * N_q + qi; to_call() brings O and L to the call's
(B, H, N_q, ...)."""
import torch

import mla_probe as M
from oracle import fa2_decode_probe as D

S_K = 2560
LENS = (0, 1, 63, 64, 65, 1000, 2049, 2560)
SPLITS = (0, 1, 3, 16, 128)
B = len(LENS)
EMPTY_B, LATE_B = 3, 5  # a list without a valid entry; a list whose valid entries all sit behind slot 64 (topk > 64)
NO_KEY = lambda nk: (-1, nk, S_K + 5, 2 ** 31 - 1, -2 ** 31)
# (H, N_q, topk): a quarter tile, a partial tile, one tile and two tiles of heads; every topk and N_q of the grid
CONFIGS = [(16, 1, 1), (40, 2, 63), (64, 3, 64), (128, 2, 65), (16, 3, 200), (128, 1, 2048), (40, 3, 2048), (128, 3, 200)]
PLANTS = ("off_by_one", "invalid_as_key_0", "decoy_accepted", "past_topk_read", "drop_last_partial", "boundary_twice", "boundary_skipped",
          "previous_position", "second_tile_other_position", "other_sequence", "wrong_page_size", "physical_row")
PAGE, WRONG_PAGE = 16, 64


def cases(rotation=0):
    """(H, N_q, topk, num_splits): every configuration under one split count, rotating with `rotation`"""
    return [cfg + (SPLITS[(k + rotation) % len(SPLITS)],) for k, cfg in enumerate(CONFIGS)]


def latent_cache(device=None):
    return M.latent_cache(LENS, S_K, device)


def lists(n_q, topk, device=None):
    """int32 (B, 1, N_q, topk)"""
    g = torch.Generator().manual_seed(1000 * n_q + topk)
    idx = torch.empty(B, 1, n_q, topk, dtype=torch.int64)
    for b, nk in enumerate(LENS):
        bad = torch.tensor(NO_KEY(nk))
        for qi in range(n_q):
            perm = torch.randperm(max(nk, 1), generator=g)[:topk]
            row = bad[torch.randint(0, len(bad), (topk,), generator=g)]          # every slot no key ...
            take = torch.rand(topk, generator=g) < 0.8                            # ... but four in five, while positions last
            take &= torch.cumsum(take, 0) <= (perm.numel() if nk else 0)
            if qi == 0 and b == EMPTY_B:
                take[:] = False
            if qi == 0 and b == LATE_B and topk > 64:
                take[:64] = False
            row[take] = perm[:int(take.sum())]
            idx[b, 0, qi] = row
    return idx.to(torch.int32).to(device)


def valid(idx, lens=LENS):
    """(B, 1, N_q, topk) bool: the slots that are keys of their sequence (lens: the B lengths, this batch's by default)"""
    nk = torch.tensor(list(lens), device=idx.device).view(len(lens), 1, 1, 1)
    return (idx >= 0) & (idx < nk)


def gathered_queries(H, n_q, uniform=False, device=None):
    """(B * N_q, 1, H, 576) in float64: pseudo-sequence (b, qi) holds the rows r = h N_q + qi of mla_probe.queries"""
    Q = M.queries(H, n_q, uniform, B, device)                                     # (B, 1, H N_q, 576), r = h N_q + qi
    return Q.view(B, H, n_q, M.D_QK).permute(0, 2, 1, 3).reshape(B * n_q, 1, H, M.D_QK)


def gather(rows, src, keep, H):
    """rows (B, n, 576): the rows a sequence can reach; src, keep (B, 1, N_q, T): the row every slot reads and whether it counts ->
    K (B * N_q, 1, T, 576), keep (B * N_q, 1, H, T).  A slot that does not count reads row 0.  B is src's."""
    B, n_q, T = src.shape[0], src.shape[2], src.shape[3]
    s = torch.where(keep, src, torch.zeros_like(src)).long().view(B, n_q * T)
    K = torch.gather(rows, 1, s.unsqueeze(-1).expand(-1, -1, rows.shape[-1])).view(B * n_q, 1, T, rows.shape[-1])
    return K, keep.reshape(B * n_q, 1, 1, T).expand(-1, -1, H, -1)


def to_call(x, n_q):
    """(B * N_q, 1, H, ...) -> (B, H, N_q, ...)"""
    return x.view(B, n_q, *x.shape[2:]).transpose(1, 2)


def truth(Q, K, keep, dtype):
    """fp64 O (B * N_q, 1, H, 512), L (B * N_q, 1, H, 1)"""
    return M.mla_truth(Q, K, keep, dtype)


def restate(Q, K, keep, num_splits, dtype):
    """emulate_split over the slots -> O, L in the I/O dtype"""
    return M.restate(Q, K, M.value_of(K), keep, [K.shape[2]] * K.shape[0], num_splits, dtype)


def pool(KV, page=PAGE, seed=7, spare=5, decoy=0):
    """the contiguous cache (B, H_kv, S_k, 576) scattered into a pool of B * max_blocks + spare pages under a seeded permutation ->
    (pool (num_blocks, H_kv, page, 576), table (B, max_blocks) int32); rows of a last page past S_k and the spare pages hold decoys (the
    rows of sequence `decoy`, whose length is 0).  B, H_kv and S_k are KV's."""
    B, h_kv, s_k = KV.shape[:3]
    mb = -(-s_k // page)
    nb = B * mb + spare
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).to(KV.device)
    table = perm[:B * mb].view(B, mb)
    padded = KV[decoy:decoy + 1, :, :1].expand(B, h_kv, mb * page, KV.shape[-1]).clone()
    padded[:, :, :s_k] = KV
    pl = torch.empty(nb, h_kv, page, KV.shape[-1], dtype=KV.dtype, device=KV.device)
    pl[table.reshape(-1)] = padded.view(B, h_kv, mb, page, -1).permute(0, 2, 1, 3, 4).reshape(B * mb, h_kv, page, -1)
    pl[perm[B * mb:]] = KV[decoy, :, :page].unsqueeze(0).expand(spare, -1, -1, -1)
    return pl, table.to(torch.int32).contiguous()


def planted(name, KV, idx, H, num_splits=3):
    """(K, keep) the restatement gathers under the planted error `name`, or None where the plant cannot apply to this configuration:
      off_by_one                  every key read one row further
      invalid_as_key_0            a slot that is no key read as key 0 (and counted)
      decoy_accepted              the entry N_k(b) taken for a key: the decoy row behind the sequence
      past_topk_read              the last tile read in full: slots topk .. of the flat index array (the next list's, the last one's: 0)
      drop_last_partial           the slots from topk - topk % 64 on not read
      boundary_twice / _skipped   the first slot of split 1 (of num_splits) taken by split 0 as well / by neither
      previous_position           position qi answered with the list of qi - 1 (cyclic)
      second_tile_other_position  heads 64.. answered with the list of position qi + 1 (cyclic)
      other_sequence              sequence b reads the list of b + 1 (cyclic) against its own rows and length
      wrong_page_size             row j % WRONG_PAGE of the page of j / PAGE (into the pages behind it in the pool)
      physical_row                the entry taken as a row of the pool, no table"""
    n_q, topk = idx.shape[2], idx.shape[3]
    rows, keep, src = KV[:, 0], valid(idx), idx
    nk = torch.tensor(LENS, device=idx.device).view(B, 1, 1, 1)
    if name == "off_by_one":
        src = (idx + 1).clamp(max=S_K - 1)
    elif name == "invalid_as_key_0":
        src, keep = torch.where(keep, idx, torch.zeros_like(idx)), torch.ones_like(keep)
    elif name == "decoy_accepted":
        keep = keep | ((idx == nk) & (idx < S_K))
    elif name == "past_topk_read":
        extra = -topk % 64
        if not extra:
            return None
        flat = torch.cat([idx.reshape(-1), torch.zeros(extra, dtype=idx.dtype, device=idx.device)])
        at = (torch.arange(B * n_q, device=idx.device) * topk).view(-1, 1) + torch.arange(topk + extra, device=idx.device)
        src = flat[at].view(B, 1, n_q, topk + extra)
        keep = (src >= 0) & (src < nk)
    elif name == "drop_last_partial":
        if not topk % 64:
            return None
        keep = keep.clone()
        keep[..., topk - topk % 64:] = False
    elif name in ("boundary_twice", "boundary_skipped"):
        c = D.split_chunk(topk, num_splits)
        if c >= topk:
            return None
        if name == "boundary_skipped":
            keep = keep.clone()
            keep[..., c] = False
        else:
            src, keep = torch.cat([idx, idx[..., c:c + 1]], -1), torch.cat([keep, keep[..., c:c + 1]], -1)
    elif name == "previous_position":
        if n_q < 2:
            return None
        src = idx.roll(1, 2)
        keep = valid(src)
    elif name == "other_sequence":
        src = idx.roll(-1, 0)
        keep = valid(src)
    elif name in ("wrong_page_size", "physical_row"):
        pl, table = pool(KV)
        rows = pl.view(1, -1, KV.shape[-1]).expand(B, -1, -1)
        j = torch.where(keep, idx, torch.zeros_like(idx)).long()
        if name == "physical_row":
            src = j
        else:
            page = torch.gather(table.long(), 1, (j // PAGE).view(B, -1)).view(j.shape)
            src = (page * PAGE + j % WRONG_PAGE).clamp(max=rows.shape[1] - 1)
    elif name == "second_tile_other_position":
        if n_q < 2 or H <= 64:
            return None
        K0, k0 = gather(rows, idx, keep, H)
        K1, k1 = gather(rows, idx.roll(-1, 2), valid(idx.roll(-1, 2)), H)
        return (K0, k0), (K1, k1)   # heads 0..63 from the first, 64.. from the second
    else:
        raise ValueError(name)
    return gather(rows, src, keep, H)


def planted_outputs(name, fn, Q, KV, idx, H, num_splits=3):
    """(O, L) of fn(Q, K, keep) -- the truth or the restatement -- under the plant, or None where it cannot apply"""
    got = planted(name, KV, idx, H, num_splits)
    if got is None:
        return None
    if name == "second_tile_other_position":
        (K0, k0), (K1, k1) = got
        (O0, L0), (O1, L1) = fn(Q, K0, k0), fn(Q, K1, k1)
        return torch.cat([O0[:, :, :64], O1[:, :, 64:]], 2), torch.cat([L0[:, :, :64], L1[:, :, 64:]], 2)
    return fn(Q, *got)
