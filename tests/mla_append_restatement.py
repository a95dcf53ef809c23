"""The latent-cache append (fa2_kvcache_mla_append, fa2_kvcache_mla_append_varlen) restated in torch on the CPU, from the pieces of
decode_append_restatement.py: the yardstick of tests/test_decode_mla_append_*.py.  No test lives here.  Everything is compared
through integer views, so caches may hold any bit pattern."""
import torch

from flash_attention_dlrs_amd.flash_attention_wrappers import FP8_CACHE_DTYPES, _rotary

from decode_append_restatement import bits, new_lengths, rows_to_store


def expected_mla_append(KV0, c_new, pe_new, lens, d_v, table=None, descale=None, cos=None, sin=None, interleaved=False):
    """(KV, start, seqlens_out) after the append, all on the CPU: a clone of KV0 -- the (B, H_kv, S_k, d) cache, or with `table` the
    (num_blocks, H_kv, page_size, d) pool -- with the new rows at the key indices start(b) + t < capacity.  A row is c_new
    (B, H_kv, N_new, d_v) followed by pe_new (B, H_kv, N_new, d - d_v) whose first rotary_dim columns are rotated at start(b) + t,
    put together in fp32 (fp64 for fp64) and rounded ONCE to the cache's dtype; for an fp8 cache (x / descale).clamp(+-max).to(fp8)
    of the unrounded value."""
    B, _, n_new, _ = c_new.shape
    assert c_new.shape[3] == d_v and c_new.shape[3] + pe_new.shape[3] == KV0.shape[3]
    P = KV0.shape[2]
    cap = P if table is None else table.shape[1] * P
    start, out = new_lengths(lens, n_new, cap)
    pos = start.long()[:, None, None] + torch.arange(n_new)[None, None, :]
    wide = torch.float64 if c_new.dtype == torch.float64 else torch.float32
    pe = pe_new.to(wide) if cos is None else _rotary(pe_new, cos, sin, pos, interleaved)
    row = torch.cat([c_new.to(wide), pe], dim=-1)
    # (widening is exact, so the one rounding leaves every column that was only copied as it was)
    rows = rows_to_store(row, KV0.dtype, descale) if KV0.dtype in FP8_CACHE_DTYPES else row.to(KV0.dtype)
    KV = KV0.clone()
    cache, rows = bits(KV), bits(rows)
    for b in range(B):
        for t in range(n_new):
            j = int(start[b]) + t
            if j >= cap:
                break  # dropped
            if table is None:
                cache[b, :, j] = rows[b, :, t]
            else:
                page = min(max(int(table[b, j // P]), 0), KV0.shape[0] - 1)
                cache[page, :, j % P] = rows[b, :, t]
    return KV, start, out


def expected_mla_append_packed(KV0, c_new, pe_new, cu, max_new, lens, d_v, table=None, descale=None, cos=None, sin=None,
                               interleaved=False):
    """(KV, seqlens_out) of the packed form: c_new (total_new, H_kv, d_v), pe_new (total_new, H_kv, d - d_v) over the offsets cu;
    sequence b brings its first min(cu[b + 1] - cu[b], max_new) rows, appended as expected_mla_append appends them."""
    B = cu.numel() - 1
    cap = KV0.shape[2] if table is None else table.shape[1] * KV0.shape[2]
    KV = KV0.clone()
    out = lens.to(torch.int64).clamp(0, cap).to(torch.int32)
    for b in range(B):
        s, n = int(cu[b]), min(int(cu[b + 1]) - int(cu[b]), max_new)
        if n <= 0:
            continue
        fixed = lambda x: x[s:s + n].transpose(0, 1).unsqueeze(0)
        ds = None if descale is None else torch.broadcast_to(descale, (B, c_new.shape[1]))[b:b + 1]
        if table is None:
            KV[b:b + 1], _, o = expected_mla_append(KV[b:b + 1], fixed(c_new), fixed(pe_new), lens[b:b + 1], d_v, None, ds, cos, sin, interleaved)
        else:
            KV, _, o = expected_mla_append(KV, fixed(c_new), fixed(pe_new), lens[b:b + 1], d_v, table[b:b + 1], ds, cos, sin, interleaved)
        out[b] = o[0]
    return KV, out
