"""The cache append (fa2_kvcache_append) restated in torch on the CPU: the yardstick of tests/test_decode_append_*.py.  No test
lives here.  Everything is compared through integer views, so caches may hold any bit pattern, NaN encodings included."""
import torch

from flash_attention_dlrs_amd.flash_attention_wrappers import FP8_CACHE_DTYPES, _rotary

INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """A tensor as integers of its element size: equality of bits, not of values."""
    return t.view(INT_VIEW[t.element_size()])


def new_lengths(lens, n_new, cap):
    """(start, seqlens_out) of the append: start = clamp(lens, 0, cap), seqlens_out = min(start + n_new, cap), int32."""
    start = lens.to(torch.int64).clamp(0, cap)
    return start.to(torch.int32), (start + n_new).clamp(max=cap).to(torch.int32)


def rows_to_store(x_new, cache_dtype, descale=None, cos=None, sin=None, positions=None, interleaved=False):
    """What the append stores for x_new (B, H_kv, N_new, d): rotated at `positions` (B, 1, N_new) when cos / sin are given, then
    rounded once to the cache's dtype -- for an fp8 cache (x_fp32 / descale).clamp(+-max).to(fp8) of the unrounded fp32 value."""
    wide = _rotary(x_new, cos, sin, positions, interleaved) if cos is not None else None
    if cache_dtype not in FP8_CACHE_DTYPES:
        return x_new.clone() if wide is None else wide.to(cache_dtype)
    wide = x_new.to(torch.float32) if wide is None else wide
    if descale is not None:
        wide = wide / torch.broadcast_to(descale, x_new.shape[:2])[:, :, None, None]
    top = torch.finfo(cache_dtype).max
    return wide.clamp(-top, top).to(cache_dtype)


def expected_append(K0, V0, k_new, v_new, lens, table=None, kd=None, vd=None, cos=None, sin=None, interleaved=False):
    """(K, V, start, seqlens_out) after the append, all on the CPU: clones of K0 / V0 -- the (B, H_kv, S_k, d) cache, or with `table`
    the (num_blocks, H_kv, page_size, d) pool -- with the stored rows at the key indices start(b) + t < capacity."""
    B, _, n_new, _ = k_new.shape
    P = K0.shape[2]
    cap = P if table is None else table.shape[1] * P
    start, out = new_lengths(lens, n_new, cap)
    pos = start.long()[:, None, None] + torch.arange(n_new)[None, None, :]
    k_rows = rows_to_store(k_new, K0.dtype, kd, cos, sin, pos, interleaved)
    v_rows = rows_to_store(v_new, V0.dtype, vd)
    K, V = K0.clone(), V0.clone()
    for cache, rows in ((bits(K), bits(k_rows)), (bits(V), bits(v_rows))):
        for b in range(B):
            for t in range(n_new):
                j = int(start[b]) + t
                if j >= cap:
                    break  # dropped
                if table is None:
                    cache[b, :, j] = rows[b, :, t]
                else:
                    page = min(max(int(table[b, j // P]), 0), K0.shape[0] - 1)
                    cache[page, :, j % P] = rows[b, :, t]
    return K, V, start, out
