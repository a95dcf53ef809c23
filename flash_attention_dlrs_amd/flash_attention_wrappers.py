"""Plain-function surface -- counterpart of the reference's src/flash_attention_wrappers.py.

flash_attention_forward(Q, K, V, dev) -> (O, L) is the entry point of the reference's correctness
script (src/test_correctness.py:34) and the only place the log2-domain log-sum-exp L is exposed.
"""
import torch

from . import _lib, autotune
from .flash_attention_torch import (MIN_TENSOR_SIZE, backward_native, convert_triton_dtype, forward_head_size,
                                    gqa_kv_heads, mla_prefill_backward, mla_prefill_forward, next_power_of_2, normalize_window, pad_last_dim,
                                    varlen_backward, varlen_forward, window_head_size)


def flash_attention_forward(Q, K, V, dev, *, causal=False, scale=1.0, variant="auto", window=None):
    # Takes tensors of shape (B, H, N, d): batch, heads, context size, head dimension
    # (reference wrappers.py:14-22: bare asserts, kept).
    # window = (left, right): local attention (FlashAttention's docstring; include/fa2_fwd.h fa2_fwd_window).
    # K and V may have H_kv heads dividing H (grouped-query attention; gqa_kv_heads raises ValueError otherwise)
    assert Q.dim() == 4
    assert K.dim() == 4 and K.shape == V.shape and Q.shape[0] == K.shape[0] and Q.shape[2:] == K.shape[2:]
    assert Q.dtype == K.dtype and K.dtype == V.dtype
    gqa_kv_heads(Q, K, V)

    B, H, N, d = Q.shape
    if window is not None:
        causal, window = normalize_window(N, causal, window)
        if window is not None:
            return _forward_window(Q, K, V, dev, scale, variant, window)

    # The reference pads Q, K, V to next_pow2(d) here (wrappers.py:27-34) and slices O afterwards; the kernels take any d
    # (SURVEY section 8 row f2): head sizes the matrix cores take run as they are (nothing copied, O has exactly d columns), the
    # others are padded as the reference pads them -- 60-90 times faster than the VALU kernel they would fall to
    # (forward_head_size).  A forced variant gets the tensors as they are.
    d_out = d
    if variant == "auto":
        d = forward_head_size(Q.dtype, B, H, N, d, causal)
        if d != d_out:
            Q, K, V = (pad_last_dim(t, d) for t in (Q, K, V))

    # Always-contiguous outputs (reference wrappers.py:37-38)
    O = torch.empty(B, H, N, d, dtype=Q.dtype, device=dev)
    L = torch.empty(B, H, N, 1, dtype=Q.dtype, device=dev)

    dtype = convert_triton_dtype(Q.dtype)
    if O.device != Q.device:   # the launch runs on Q's device: an O allocated elsewhere would be a foreign pointer there
        raise ValueError(f"dev={dev} is not the device of Q, K, V ({Q.device})")
    v = _lib.VARIANTS[variant]
    if variant == "auto" and autotune.enabled() and K.shape[1] == H:  # (the tuner's key does not see H_kv)
        v = autotune.pick(Q, K, V, O, L, dtype, causal, scale)  # the on-box tuner, FA2_AUTOTUNE=1
        if v != _lib.VARIANT_AUTO:
            try:
                _lib.fa2_fwd(Q, K, V, O, L, dtype, causal=causal, scale=scale, variant=v)
                return O[..., :d_out], L
            except TypeError:
                # the tuned variant cannot run THIS problem (strides, alignment, N * stride >= 2 GiB: the tuner's key does
                # not see them): the static table can, it falls back to the kernels that take any layout
                v = _lib.VARIANT_AUTO
    _lib.fa2_fwd(Q, K, V, O, L, dtype, causal=causal, scale=scale, variant=v)

    return O[..., :d_out], L     # (reference wrappers.py:63)


def _forward_window(Q, K, V, dev, scale, variant, window):
    """Local attention with a normalised window: contiguous O, padded like the plain path where the windowed matrix kernel
    wants it (auto only; a forced variant gets the tensors as they are); the autotuner is not consulted."""
    B, H, N, d_out = Q.shape
    d = d_out
    if variant == "auto":
        d = window_head_size(Q.dtype, d_out)
        if d != d_out:
            Q, K, V = (pad_last_dim(t, d) for t in (Q, K, V))
    O = torch.empty(B, H, N, d, dtype=Q.dtype, device=dev)
    L = torch.empty(B, H, N, 1, dtype=Q.dtype, device=dev)
    dtype = convert_triton_dtype(Q.dtype)
    if O.device != Q.device:
        raise ValueError(f"dev={dev} is not the device of Q, K, V ({Q.device})")
    _lib.fa2_fwd(Q, K, V, O, L, dtype, causal=False, scale=scale, variant=_lib.VARIANTS[variant], window=window)
    if d != d_out:
        O = O[..., :d_out].contiguous()
    return O, L


def flash_attention_backward(Q, K, V, O, dO, L, dev, deterministic=False, *, causal=False, scale=1.0, variant="auto",
                             window=None):
    """(dQ, dK, dV) through the native backward kernels (include/fa2_bwd.h).  Same signature as the reference
    (wrappers.py:66-75); `deterministic` selects between two kernels there -- here the one implementation is
    deterministic by construction, so the flag is accepted and ignored.  d is padded like in the forward
    (wrappers.py:91-104) and the gradients are returned as [:d] views."""
    assert Q.dim() == 4
    assert K.dim() == 4 and K.shape == V.shape and Q.shape[0] == K.shape[0] and Q.shape[2:] == K.shape[2:]
    assert O.shape == Q.shape and dO.shape == Q.shape
    assert Q.dtype == K.dtype and K.dtype == V.dtype and Q.dtype == dO.dtype
    gqa_kv_heads(Q, K, V)
    d = Q.shape[-1]
    d_pow = max(next_power_of_2(d), MIN_TENSOR_SIZE)
    if d_pow != d:
        Q, K, V, O, dO = (pad_last_dim(t, d_pow) for t in (Q, K, V, O, dO))
    dQ, dK, dV = backward_native(Q, K, V, O, dO, L, causal=causal, scale=scale, variant=variant, window=window)
    return dQ[..., :d], dK[..., :d], dV[..., :d]


def flash_attention_varlen_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dev, *, causal=False,
                                   scale=1.0, window=None, variant="auto"):
    """Packed variable-length forward (include/fa2_fwd.h fa2_fwd_varlen) -> (O, L): Q (total_q, H, d), K / V (total_k, H, d)
    or (total_k, H_kv, d) with H_kv dividing H (grouped-query, fa2_fwd_varlen_gqa), cu_seqlens int32 (B + 1) on Q's device;
    O (total_q, H, d), L (H, total_q).  The autotuner is not consulted."""
    if Q.device != torch.device(dev):
        raise ValueError(f"dev={dev} is not the device of Q, K, V ({Q.device})")
    return varlen_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal, scale=scale,
                          window=window, variant=variant)


def flash_attention_varlen_backward(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dev, *,
                                    causal=False, scale=1.0, window=None, variant="auto"):
    """(dQ, dK, dV) of flash_attention_varlen_forward (include/fa2_bwd.h fa2_bwd_varlen, fa2_bwd_varlen_gqa); deterministic.
    dK and dV have K's and V's shapes: (total_k, H_kv, d) for grouped-query K / V, summed over each group in the kernel."""
    if Q.device != torch.device(dev):
        raise ValueError(f"dev={dev} is not the device of Q, K, V ({Q.device})")
    return varlen_backward(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal,
                           scale=scale, window=window, variant=variant)


def flash_attention_mla_prefill_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dev, *, causal=False,
                                        scale=1.0, window=None, variant="auto"):
    """Packed forward with a value head size of its own (include/fa2_fwd.h fa2_fwd_varlen_dv) -> (O, L): un-absorbed MLA prefill,
    Q (total_q, H, d), K (total_k, H_kv, d), V (total_k, H_kv, d_v) with H_kv dividing H, cu_seqlens int32 (B + 1) on Q's device;
    O (total_q, H, d_v) contiguous, L (H, total_q).  Strided inputs are passed through -- the two views of a fused (total, H,
    192 + 128) up-projection buffer are a valid K and V -- and no head size is padded: "auto" runs the matrix kernel for f16 / bf16
    at d 192 / d_v 128 and the VALU kernel on anything else, "generic" and "mfma16dv" force one (_lib.VARLEN_DV_VARIANTS)."""
    if Q.device != torch.device(dev):
        raise ValueError(f"dev={dev} is not the device of Q, K, V ({Q.device})")
    return mla_prefill_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal, scale=scale,
                               window=window, variant=variant)


def flash_attention_mla_prefill_backward(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dev, *,
                                         causal=False, scale=1.0, window=None, variant="auto"):
    """(dQ, dK, dV) of flash_attention_mla_prefill_forward (include/fa2_bwd.h fa2_bwd_varlen_dv) with Q's, K's and V's shapes;
    deterministic.  O and dO are (total_q, H, d_v), L (H, total_q); dK and dV are summed over each group of query heads in the
    kernel.  Strided tensors are passed through and no head size is padded: "auto" runs the matrix kernel for f16 / bf16 at d 192 /
    d_v 128 and the VALU kernel on anything else, "generic" and "mfma16dv" force one (_lib.BWD_VARLEN_DV_VARIANTS)."""
    if Q.device != torch.device(dev):
        raise ValueError(f"dev={dev} is not the device of Q, K, V ({Q.device})")
    return mla_prefill_backward(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal,
                                scale=scale, window=window, variant=variant)


FP8_CACHE_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)


def quantize_kv_cache(K, dtype):
    """(K8, descale) of a (B, H_kv, S_k, d) cache for flash_attention_kvcache_forward's fp8 mode: one scale per (b, h_kv),
    descale = amax over (S_k, d) / finfo(dtype).max (1 where the head is all zeros), float32 (B, H_kv); K8 = (K / descale) in dtype
    (torch.float8_e4m3fn or torch.float8_e5m2).  Plain torch, any device."""
    if dtype not in FP8_CACHE_DTYPES:
        raise ValueError(f"quantize_kv_cache: dtype must be torch.float8_e4m3fn or torch.float8_e5m2, got {dtype}")
    if K.dim() != 4:
        raise ValueError(f"quantize_kv_cache: the cache must be (B, H_kv, S_k, d), got {tuple(K.shape)}")
    top = torch.finfo(dtype).max
    amax = K.detach().abs().amax(dim=(2, 3)).to(torch.float32)
    descale = torch.where(amax > 0, amax / top, torch.ones_like(amax))
    K8 = (K.to(torch.float32) / descale[:, :, None, None]).clamp(-top, top).to(dtype)
    return K8, descale


def dequantize_kv_cache(K8, descale, dtype):
    """The inverse of quantize_kv_cache: descale * float(K8) in dtype; descale broadcasts to (B, H_kv)."""
    B, H_kv = K8.shape[:2]
    return (K8.to(torch.float32) * torch.broadcast_to(descale.to(torch.float32), (B, H_kv))[:, :, None, None]).to(dtype)


def _kvcache_descale(name, t, Q, B, H_kv):
    """A descale argument as a (B, H_kv) view whose strides the C ABI takes (0 on broadcast axes)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"kvcache: {name} must be a float32 tensor (or None)")
    if t.device != Q.device:
        raise ValueError(f"kvcache: {name} must be on Q's device ({Q.device}), got {t.device}")
    try:
        return torch.broadcast_to(t, (B, H_kv))
    except RuntimeError:
        raise ValueError(f"kvcache: {name} of shape {tuple(t.shape)} does not broadcast to (B, H_kv) = ({B}, {H_kv})") from None


def _descale_views(k_descale, v_descale, Q, B, H_kv):
    """Both descales as the launchers' keywords."""
    return dict(k_descale=_kvcache_descale("k_descale", k_descale, Q, B, H_kv), v_descale=_kvcache_descale("v_descale", v_descale, Q, B, H_kv))


def _check_cache_seqlens(cache_seqlens, B, anchor, name, or_none=""):
    """cache_seqlens beside the tensor `anchor`, called `name` in the messages, whose device it must share."""
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 \
            or not cache_seqlens.is_contiguous() or cache_seqlens.numel() != B:
        raise ValueError(f"kvcache: cache_seqlens must be a contiguous int32 tensor of B = {B} entries{or_none}")
    if cache_seqlens.device != anchor.device:
        raise ValueError(f"kvcache: cache_seqlens must be on {name}'s device ({anchor.device}), got {cache_seqlens.device}")


def _check_block_table(block_table, B, page_size, anchor, name):
    """block_table over pages of page_size rows, beside the tensor `anchor`, called `name` in the messages."""
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 \
            or block_table.shape[0] != B or block_table.shape[1] < 1:
        raise ValueError(f"kvcache: block_table must be an int32 tensor (B, max_blocks) with B = {B}, max_blocks >= 1")
    if block_table.stride(1) != 1 or block_table.stride(0) < 0:
        raise ValueError(f"kvcache: block_table needs unit stride in its last axis, got strides {tuple(block_table.stride())}")
    if block_table.device != anchor.device:
        raise ValueError(f"kvcache: block_table must be on {name}'s device ({anchor.device}), got {block_table.device}")
    if block_table.shape[1] * page_size > 1 << 28:
        raise ValueError(f"kvcache: the capacity max_blocks * page_size must be <= 2^28, got {block_table.shape[1]} * {page_size}")


def _capacity(K_cache, block_table):
    return K_cache.shape[2] if block_table is None else block_table.shape[1] * K_cache.shape[2]


def _kvcache_outputs(Q, o_shape, l_shape, workspace_bytes):
    """(O, L, workspace) of a cache call, allocated: the fp32 workspace of workspace_bytes bytes, None for 0 (a single split)."""
    O = torch.empty(o_shape, dtype=Q.dtype, device=Q.device)
    L = torch.empty(l_shape, dtype=Q.dtype, device=Q.device)
    ws = torch.empty(workspace_bytes // 4, dtype=torch.float32, device=Q.device) if workspace_bytes else None
    return O, L, ws


def _check_dev(dev, Q, K_cache, V_cache):
    if Q.device != torch.device(dev) or K_cache.device != Q.device or V_cache.device != Q.device:
        raise ValueError(f"dev={dev} is not the device of Q, K_cache, V_cache ({Q.device}, {K_cache.device}, {V_cache.device})")


def apply_rotary(x, cos, sin, positions, interleaved=False):
    """Rotary embedding as the cache append applies it (include/fa2_fwd.h fa2_kvcache_append), in plain torch on any device: the
    meaning of flash_attention_kvcache_forward's rotary_cos / rotary_sin and the yardstick of its tests, bit for bit.  x (..., d);
    cos, sin (S_rot, rotary_dim / 2) with rotary_dim even and <= d; positions: an int tensor broadcasting to x.shape[:-1], clamped
    to [0, S_rot - 1].  interleaved=False pairs column i with i + rotary_dim / 2 (GPT-NeoX), True pairs 2i with 2i + 1 (GPT-J);
    columns >= rotary_dim pass through.  (x1, x2) -> (x1 c - x2 s, x2 c + x1 s) in float32 (float64 for float64 input), every
    product, sum and difference rounded on its own, then one rounding to x.dtype."""
    return _rotary(x, cos, sin, positions, interleaved).to(x.dtype)


def _rotary(x, cos, sin, positions, interleaved):
    """apply_rotary before the last rounding: float32 (float64 for float64 x), what an fp8 cache quantises."""
    half = cos.shape[-1]
    rd = 2 * half
    if cos.dim() != 2 or cos.shape != sin.shape or half < 1 or rd > x.shape[-1]:
        raise ValueError(f"apply_rotary: cos, sin must be (S_rot, rotary_dim / 2) of one shape with 2 <= rotary_dim <= d = "
                         f"{x.shape[-1]}, got {tuple(cos.shape)}, {tuple(sin.shape)}")
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    pos = torch.broadcast_to(torch.as_tensor(positions, device=x.device).long().clamp(0, cos.shape[0] - 1), x.shape[:-1])
    c, s = cos.to(wide)[pos], sin.to(wide)[pos]  # (..., rotary_dim / 2)
    xw = x.to(wide)
    x1, x2 = (xw[..., 0:rd:2], xw[..., 1:rd:2]) if interleaved else (xw[..., :half], xw[..., half:rd])
    o1 = x1 * c - x2 * s  # (torch rounds each of these operations on its own)
    o2 = x2 * c + x1 * s
    out = xw.clone()
    if interleaved:
        out[..., 0:rd:2], out[..., 1:rd:2] = o1, o2
    else:
        out[..., :half], out[..., half:rd] = o1, o2
    return out


def check_kvcache_append_args(K_cache, V_cache, k_new, v_new, cache_seqlens, k_descale=None, v_descale=None, block_table=None,
                              rotary_cos=None, rotary_sin=None, Q=None):
    """ValueError for what kvcache_append (and the append keywords of flash_attention_kvcache_forward) cannot take.  Pure: takes CPU
    tensors as well."""
    if (k_new is None) != (v_new is None):
        raise ValueError("kvcache: k_new and v_new go together")
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError("kvcache: rotary_cos and rotary_sin go together")
    if k_new is None:
        if rotary_cos is not None:
            raise ValueError("kvcache: rotary_cos / rotary_sin need k_new and v_new (the rotation is part of the cache update)")
        return
    if cache_seqlens is None:
        raise ValueError("kvcache: k_new / v_new need cache_seqlens (the position the new tokens go to)")
    if not isinstance(k_new, torch.Tensor) or not isinstance(v_new, torch.Tensor) or k_new.dim() != 4 or k_new.shape != v_new.shape \
            or K_cache.dim() != 4 or K_cache.shape != V_cache.shape or k_new.shape[1] != K_cache.shape[1] \
            or k_new.shape[3] != K_cache.shape[3] or k_new.shape[2] < 1 or (block_table is None and k_new.shape[0] != K_cache.shape[0]):
        raise ValueError(f"kvcache: k_new, v_new must be (B, H_kv, N_new, d) of one shape with N_new >= 1, B, H_kv and d the cache's: "
                         f"got k_new {tuple(k_new.shape)}, v_new {tuple(v_new.shape)}, K_cache {tuple(K_cache.shape)}, V_cache "
                         f"{tuple(V_cache.shape)}")
    B, H_kv = k_new.shape[:2]
    if k_new.dtype != v_new.dtype or K_cache.dtype != V_cache.dtype:
        raise ValueError("kvcache: k_new and v_new, and K_cache and V_cache, must have the same dtype")
    if k_new.dtype in FP8_CACHE_DTYPES:
        raise ValueError(f"kvcache: dtype {k_new.dtype} is not supported for k_new, v_new (an fp8 cache takes float16 / bfloat16)")
    if K_cache.dtype in FP8_CACHE_DTYPES:
        if k_new.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"kvcache: an fp8 cache needs k_new, v_new in float16 or bfloat16, got {k_new.dtype}")
        _kvcache_descale("k_descale", k_descale, k_new, B, H_kv)
        _kvcache_descale("v_descale", v_descale, k_new, B, H_kv)
    else:
        if k_new.dtype != K_cache.dtype:
            raise ValueError("kvcache: k_new, v_new must have the cache's dtype (or the cache an fp8 dtype under 16-bit k_new, v_new)")
        if k_descale is not None or v_descale is not None:
            raise ValueError(f"kvcache: k_descale / v_descale go with an fp8 cache, not with {K_cache.dtype}")
    convert_triton_dtype(k_new.dtype)
    if Q is not None and Q.dtype != k_new.dtype:
        raise ValueError("kvcache: k_new, v_new must have Q's dtype")
    for name, t in (("v_new", v_new), ("K_cache", K_cache), ("V_cache", V_cache)):
        if t.device != k_new.device:
            raise ValueError(f"kvcache: {name} must be on k_new's device ({k_new.device}), got {t.device}")
    _check_cache_seqlens(cache_seqlens, B, k_new, "k_new")
    if block_table is not None:
        _check_block_table(block_table, B, K_cache.shape[2], k_new, "k_new")
    if rotary_cos is not None:
        _check_rotary_tables(rotary_cos, rotary_sin, k_new.shape[3], f"d = {k_new.shape[3]}", k_new, "k_new")


def _check_rotary_tables(rotary_cos, rotary_sin, limit, bound, anchor, anchor_name):
    """rotary_cos, rotary_sin beside the new tokens `anchor`, called `anchor_name` in the messages: rotary_dim at most `limit`, which
    the messages spell `bound`."""
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape != rotary_cos.shape or t.shape[0] < 1 \
                or not 1 <= t.shape[1] <= limit // 2:
            raise ValueError(f"kvcache: rotary_cos, rotary_sin must be (S_rot, rotary_dim / 2) of one shape with S_rot >= 1 and "
                             f"2 <= rotary_dim <= {bound}, got {name} {tuple(t.shape) if isinstance(t, torch.Tensor) else t!r}")
        if t.dtype != anchor.dtype:
            raise ValueError(f"kvcache: {name} must have {anchor_name}'s dtype ({anchor.dtype}), got {t.dtype}")
        if t.stride(1) != 1 or t.stride(0) < 0:
            raise ValueError(f"kvcache: {name} needs unit stride in its last axis, got strides {tuple(t.stride())}")
        if t.device != anchor.device:
            raise ValueError(f"kvcache: {name} must be on {anchor_name}'s device ({anchor.device}), got {t.device}")


def kvcache_append(K_cache, V_cache, k_new, v_new, cache_seqlens, *, k_descale=None, v_descale=None, block_table=None,
                   rotary_cos=None, rotary_sin=None, rotary_interleaved=False):
    """The cache update of a decode step alone (include/fa2_fwd.h fa2_kvcache_append) -> new_seqlens, int32 (B,): what an engine
    passes as the next step's cache_seqlens.  k_new, v_new (B, H_kv, N_new, d), any strides, go into K_cache / V_cache IN PLACE at
    key indices clamp(cache_seqlens[b], 0, capacity) + t, K rotated by rotary_cos / rotary_sin at that position (apply_rotary), both
    quantised with the given descales where the cache is fp8, through block_table where it is paged; tokens past the capacity are
    dropped and new_seqlens = min(cache_seqlens + N_new, capacity).  cache_seqlens is not modified.  The arguments are
    flash_attention_kvcache_forward's; a prefill fills a cache with this call.  Two sequences that append into the same row of a
    shared page leave either one's bytes there: copy on write is the caller's."""
    if k_new is None or v_new is None:
        raise ValueError("kvcache: kvcache_append needs k_new and v_new")
    check_kvcache_append_args(K_cache, V_cache, k_new, v_new, cache_seqlens, k_descale, v_descale, block_table, rotary_cos, rotary_sin)
    B, H_kv = k_new.shape[:2]
    new_seqlens = torch.empty_like(cache_seqlens)
    _lib.fa2_kvcache_append(K_cache, V_cache, k_new, v_new, cache_seqlens, new_seqlens, convert_triton_dtype(k_new.dtype),
                            convert_triton_dtype(K_cache.dtype), block_table=block_table,
                            **_descale_views(k_descale, v_descale, k_new, B, H_kv), rotary_cos=rotary_cos,
                            rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved)
    return new_seqlens


def check_kvcache_append_varlen_args(K_cache, V_cache, k_new, v_new, cu_seqlens_new, max_seqlen_new, cache_seqlens, k_descale=None,
                                     v_descale=None, block_table=None, rotary_cos=None, rotary_sin=None, Q=None):
    """ValueError for what kvcache_append_varlen (and the append keywords of flash_attention_varlen_kvcache_forward) cannot take: the
    packed k_new / v_new, cu_seqlens_new and max_seqlen_new, and every rule of check_kvcache_append_args for the cache, its lengths,
    descales, table and rotary tables.  Q, packed (total_new, H, d), only where it is rotated along.  Pure: takes CPU tensors as
    well."""
    if (k_new is None) != (v_new is None):
        raise ValueError("varlen kvcache: k_new and v_new go together")
    if k_new is None:
        check_kvcache_append_args(K_cache, V_cache, None, None, cache_seqlens, rotary_cos=rotary_cos, rotary_sin=rotary_sin)
        return
    if not isinstance(k_new, torch.Tensor) or not isinstance(v_new, torch.Tensor) or k_new.dim() != 3 or k_new.shape != v_new.shape \
            or not 1 <= k_new.shape[0] <= 1 << 28:
        raise ValueError(f"varlen kvcache: k_new, v_new must be packed (total_new, H_kv, d) of one shape with total_new in [1, 2^28], got "
                         f"{tuple(k_new.shape) if isinstance(k_new, torch.Tensor) else type(k_new).__name__}, "
                         f"{tuple(v_new.shape) if isinstance(v_new, torch.Tensor) else type(v_new).__name__}")
    if not isinstance(cu_seqlens_new, torch.Tensor) or cu_seqlens_new.dtype != torch.int32 or cu_seqlens_new.dim() != 1 \
            or not cu_seqlens_new.is_contiguous() or cu_seqlens_new.numel() < 2:
        raise ValueError("varlen kvcache: cu_seqlens_new must be a contiguous int32 tensor of B + 1 >= 2 entries")
    if cu_seqlens_new.device != k_new.device:
        raise ValueError(f"varlen kvcache: cu_seqlens_new must be on k_new's device ({k_new.device}), got {cu_seqlens_new.device}")
    if isinstance(max_seqlen_new, bool) or not isinstance(max_seqlen_new, int) or not 1 <= max_seqlen_new <= 1 << 28:
        raise ValueError(f"varlen kvcache: max_seqlen_new must be an int in [1, 2^28], got {max_seqlen_new!r}")
    if Q is not None and (not isinstance(Q, torch.Tensor) or Q.dim() != 3 or Q.shape[0] != k_new.shape[0] or Q.shape[2] != k_new.shape[2]):
        raise ValueError(f"varlen kvcache: Q must be packed (total_new, H, d) with k_new's total_new and d, got "
                         f"{tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__} beside k_new {tuple(k_new.shape)}")
    slabs = max(2 * k_new.shape[1], 0 if Q is None else Q.shape[1])
    if k_new.shape[0] * slabs > 1 << 40:
        raise ValueError(f"varlen kvcache: total_new * max(H, 2 * H_kv) must be <= 2^40, got {k_new.shape[0]} * {slabs}")
    B = cu_seqlens_new.numel() - 1
    # the rest is the fixed call's: the tokens seen through (B, H_kv, 1, d) views (no data is read)
    as_fixed = lambda t: t[:1].transpose(0, 1).unsqueeze(0).expand(B, -1, -1, -1)
    check_kvcache_append_args(K_cache, V_cache, as_fixed(k_new), as_fixed(v_new), cache_seqlens, k_descale, v_descale, block_table,
                              rotary_cos, rotary_sin, Q)


def kvcache_append_varlen(K_cache, V_cache, k_new, v_new, cu_seqlens_new, max_seqlen_new, cache_seqlens, *, k_descale=None,
                          v_descale=None, block_table=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False):
    """kvcache_append for a ragged batch in one launch (include/fa2_fwd.h fa2_kvcache_append_varlen) -> new_seqlens, int32 (B,).
    k_new, v_new packed (total_new, H_kv, d), any strides; cu_seqlens_new int32 (B + 1,) on their device: sequence b brings the
    min(cu[b + 1] - cu[b], max_seqlen_new) rows from cu[b] on, none is legal, and row cu[b] + t becomes key
    clamp(cache_seqlens[b], 0, capacity) + t of sequence b, exactly as kvcache_append stores token t -- rotary, fp8 descales, block
    table and the drop of tokens past the capacity included.  new_seqlens[b] = min(cache_seqlens[b] + n_new(b), capacity), for
    sequences without tokens too.  Rows outside every sequence are not read; cache_seqlens is not modified.  What a mixed step of
    chunked prefill and decodes hands over as one tensor goes in as it is."""
    if k_new is None or v_new is None:
        raise ValueError("varlen kvcache: kvcache_append_varlen needs k_new and v_new")
    check_kvcache_append_varlen_args(K_cache, V_cache, k_new, v_new, cu_seqlens_new, max_seqlen_new, cache_seqlens, k_descale, v_descale,
                                     block_table, rotary_cos, rotary_sin)
    B, H_kv = cu_seqlens_new.numel() - 1, k_new.shape[1]
    new_seqlens = torch.empty_like(cache_seqlens)
    _lib.fa2_kvcache_append_varlen(K_cache, V_cache, k_new, v_new, cu_seqlens_new, max_seqlen_new, cache_seqlens, new_seqlens,
                                   convert_triton_dtype(k_new.dtype), convert_triton_dtype(K_cache.dtype), block_table=block_table,
                                   **_descale_views(k_descale, v_descale, k_new, B, H_kv), rotary_cos=rotary_cos,
                                   rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved)
    return new_seqlens


def check_kvcache_args(Q, K_cache, V_cache, cache_seqlens, window, num_splits, k_descale=None, v_descale=None, block_table=None):
    """ValueError for what flash_attention_kvcache_forward cannot take (shapes, dtypes, descales, cache_seqlens, block_table,
    window, num_splits).  Pure: takes CPU tensors as well (the CUDA-device check is the launch's)."""
    if block_table is not None:  # paged: K_cache, V_cache are pools, their leading axis counts pages, B is Q's
        if Q.dim() != 4 or K_cache.dim() != 4 or V_cache.dim() != 4 or K_cache.shape != V_cache.shape \
                or Q.shape[3] != K_cache.shape[3] or Q.shape[2] < 1 or K_cache.shape[0] < 1 or K_cache.shape[2] < 1:
            raise ValueError(f"kvcache: with block_table, Q must be (B, H, N_q, d) and K_cache, V_cache pools (num_blocks, H_kv, "
                             f"page_size, d) of one shape with N_q, num_blocks, page_size >= 1: got Q {tuple(Q.shape)}, K_cache "
                             f"{tuple(K_cache.shape)}, V_cache {tuple(V_cache.shape)}")
        _check_block_table(block_table, Q.shape[0], K_cache.shape[2], Q, "Q")
    elif Q.dim() != 4 or K_cache.dim() != 4 or V_cache.dim() != 4 or K_cache.shape != V_cache.shape \
            or Q.shape[0] != K_cache.shape[0] or Q.shape[3] != K_cache.shape[3] or Q.shape[2] < 1 or K_cache.shape[2] < 1:
        raise ValueError(f"kvcache: Q must be (B, H, N_q, d) and K_cache, V_cache (B, H_kv, S_k, d) with N_q, S_k >= 1: got Q "
                         f"{tuple(Q.shape)}, K_cache {tuple(K_cache.shape)}, V_cache {tuple(V_cache.shape)}")
    # the head rule of the dense entry points, on views that drop the sequence axis (N_q and S_k differ here)
    gqa_kv_heads(Q[:1, :, :1], K_cache[:1, :, :1], V_cache[:1, :, :1])
    if Q.dtype in FP8_CACHE_DTYPES:
        raise ValueError(f"kvcache: dtype {Q.dtype} is not supported for Q (e4m3fn cannot hold L = +inf)")
    if K_cache.dtype != V_cache.dtype:
        raise ValueError("kvcache: K_cache and V_cache must have the same dtype")
    if K_cache.dtype in FP8_CACHE_DTYPES:  # fp8 cache: Q, O, L stay 16-bit
        if Q.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"kvcache: an fp8 cache needs Q in float16 or bfloat16, got {Q.dtype}")
        _kvcache_descale("k_descale", k_descale, Q, Q.shape[0], K_cache.shape[1])
        _kvcache_descale("v_descale", v_descale, Q, Q.shape[0], K_cache.shape[1])
    else:
        if Q.dtype != K_cache.dtype:
            raise ValueError("kvcache: Q, K_cache, V_cache must have the same dtype (or the caches an fp8 dtype under 16-bit Q)")
        if k_descale is not None or v_descale is not None:
            raise ValueError(f"kvcache: k_descale / v_descale go with an fp8 cache, not with {K_cache.dtype}")
    convert_triton_dtype(Q.dtype)
    if cache_seqlens is not None:
        _check_cache_seqlens(cache_seqlens, Q.shape[0], Q, "Q", " (or None)")
    if window is not None:
        normalize_window(1, False, window)  # the sides' own rules (pair of ints >= -1); the shift is per sequence
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 0 <= num_splits <= _lib.KVCACHE_MAX_SPLITS:
        raise ValueError(f"kvcache: num_splits must be an int in [0, {_lib.KVCACHE_MAX_SPLITS}] (0 = auto), got {num_splits!r}")


def flash_attention_kvcache_forward(Q, K_cache, V_cache, cache_seqlens, dev, *, causal=False, scale=1.0, window=None, num_splits=0,
                                    variant="auto", k_descale=None, v_descale=None, block_table=None, k_new=None, v_new=None,
                                    rotary_cos=None, rotary_sin=None, rotary_interleaved=False):
    """Decode attention over a padded KV cache, split-KV (include/fa2_fwd.h fa2_fwd_kvcache) -> (O, L).  Q (B, H, N_q, d);
    K_cache, V_cache (B, H_kv, S_k, d) of capacity S_k, any strides (a flash-attn (B, S, H_kv, d) cache: pass its
    .transpose(1, 2) view), H_kv dividing H; cache_seqlens int32 (B,) on Q's device, sequence b attends to its first
    cache_seqlens[b] keys (None: all S_k).  causal / window are bottom-right aligned as in the varlen call.  O (B, H, N_q, d)
    contiguous, L (B, H, N_q) log2-domain, both in Q's dtype; rows without a visible key get O = 0, L = +inf.  num_splits = 0
    lets the library choose; variant is one of _lib.KVCACHE_VARIANTS.  No autograd, no autotuner.

    fp8 cache (fa2_fwd_kvcache_fp8): K_cache and V_cache in torch.float8_e4m3fn or torch.float8_e5m2 (both the same) under
    float16 / bfloat16 Q.  K = k_descale * float(K_cache), V = v_descale * float(V_cache) with float32 descales on Q's device that
    broadcast to (B, H_kv) (None: 1; they must be finite and > 0) -- quantize_kv_cache makes such a cache.  The arithmetic stays
    16-bit: only the cache's storage is fp8.

    Paged cache (fa2_fwd_kvcache_paged): with block_table, an int32 (B, max_blocks) tensor on Q's device with unit stride in its
    last axis, K_cache and V_cache are page pools (num_blocks, H_kv, page_size, d), any strides (a flash-attn (num_blocks,
    page_size, H_kv, d) pool: pass its .transpose(1, 2) view), in Q's dtype or fp8 with descales as above.  Key j of sequence b is
    row j % page_size of page block_table[b, j // page_size]; the capacity max_blocks * page_size takes S_k's place (cache_seqlens
    None: every sequence uses all of it).  Pages may be shared between sequences.  The table's contents are not validated (that
    would need a device synchronisation): the kernels clamp every entry they read to [0, num_blocks - 1], so a bad entry gives a
    wrong result for that sequence and never an access outside the pool; entries of pages past a sequence's length, pool pages
    no visible key maps to and the rows of a last page past the length are never read.  On the cache the pool was scattered from
    the result equals the contiguous call's bit for bit.  variant "mfma16" needs page_size % 64 == 0; "auto" takes the generic
    kernel for other page sizes.

    Append (fa2_fwd_kvcache_append): with k_new, v_new (B, H_kv, N_new, d) in Q's dtype, any strides (a flash-attn
    (B, N_new, H_kv, d) tensor: pass its .transpose(1, 2) view), the call first updates K_cache / V_cache IN PLACE as
    kvcache_append does -- the new tokens at key indices cache_seqlens[b] + t, quantised with the descales where the cache is fp8,
    through block_table where it is paged -- and then attends over cache_seqlens + N_new keys (at most the capacity: tokens past it
    are dropped).  cache_seqlens is required and not modified.  rotary_cos, rotary_sin (S_rot, rotary_dim / 2) in Q's dtype with unit
    last stride rotate K token t at position cache_seqlens[b] + t and Q (a copy: Q itself is not modified) at cache_seqlens[b] + i for
    row i when the call is causal or windowed, every row at cache_seqlens[b] otherwise, as flash-attn does; apply_rotary is the
    arithmetic, bit for bit.  They need k_new / v_new.

    Value head size d_v != d (fa2_fwd_kvcache_mla): a V_cache whose LAST axis differs from K_cache's, all other axes equal --
    V_cache (B, H_kv, S_k, d_v) or a pool (num_blocks, H_kv, page_size, d_v) -- with d in [1, 576] and d_v in [1, 512]; O is
    (B, H, N_q, d_v).  V_cache may be a view of K_cache: multi-head latent attention in its absorbed form is H_kv = 1, d = 576 and
    V_cache = K_cache[..., :512] (flash_attention_mla_decode_forward passes exactly that).  variant is then one of
    _lib.KVCACHE_MLA_VARIANTS: "mla16" (f16 / bf16, d = 576, d_v = 512, V_cache that view of K_cache, unit d-stride and 16-byte
    aligned rows, contiguous or paged with page_size % 64 == 0), "generic" (everything else), "auto".  Out of scope with d_v != d,
    each a ValueError: an fp8 cache and k_descale / v_descale (flash_attention_mla_decode_forward takes an fp8 latent cache with its
    one kv_descale), k_new / v_new (MLA rotates the last 64 columns and writes ONE tensor:
    kvcache_append does neither) and the rotary arguments; so is flash_attention_varlen_kvcache_forward."""
    if isinstance(K_cache, torch.Tensor) and isinstance(V_cache, torch.Tensor) and K_cache.dim() == 4 and V_cache.dim() == 4 \
            and K_cache.shape[:3] == V_cache.shape[:3] and K_cache.shape[3] != V_cache.shape[3]:
        return _kvcache_mla_forward(Q, K_cache, V_cache, cache_seqlens, dev, causal, scale, window, num_splits, variant, k_descale,
                                    v_descale, block_table, k_new, v_new, rotary_cos, rotary_sin)
    check_kvcache_args(Q, K_cache, V_cache, cache_seqlens, window, num_splits, k_descale, v_descale, block_table)
    check_kvcache_append_args(K_cache, V_cache, k_new, v_new, cache_seqlens, k_descale, v_descale, block_table, rotary_cos, rotary_sin,
                              Q)
    if variant not in _lib.KVCACHE_VARIANTS:
        raise ValueError(f"kvcache: variant must be one of {sorted(_lib.KVCACHE_VARIANTS)}, got {variant!r}")
    _check_dev(dev, Q, K_cache, V_cache)
    B, H, N_q, d = Q.shape
    H_kv = K_cache.shape[1]
    dtype = convert_triton_dtype(Q.dtype)
    n = num_splits or _lib.kvcache_num_splits(B, H, H_kv, N_q, _capacity(K_cache, block_table), d, dtype)
    O, L, ws = _kvcache_outputs(Q, (B, H, N_q, d), (B, H, N_q), _lib.kvcache_workspace_bytes(B, H, N_q, d, n) if n > 1 else 0)
    if k_new is not None:
        if k_new.shape[0] != B or k_new.device != Q.device:
            raise ValueError(f"kvcache: k_new, v_new must have Q's batch size {B} and device ({Q.device}), got {tuple(k_new.shape)} on "
                             f"{k_new.device}")
        _lib.fa2_fwd_kvcache_append(Q, K_cache, V_cache, O, L, k_new, v_new, cache_seqlens, torch.empty_like(cache_seqlens), dtype,
                                    convert_triton_dtype(K_cache.dtype), block_table=block_table,
                                    **_descale_views(k_descale, v_descale, Q, B, H_kv), rotary_cos=rotary_cos,
                                    rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved,
                                    q_rot=None if rotary_cos is None else torch.empty(B, H, N_q, d, dtype=Q.dtype, device=Q.device),
                                    causal=causal, scale=scale, window=window, num_splits=n, workspace=ws,
                                    variant=_lib.KVCACHE_VARIANTS[variant])
        return O, L
    if block_table is not None:
        _lib.fa2_fwd_kvcache_paged(Q, K_cache, V_cache, O, L, block_table, cache_seqlens, dtype, convert_triton_dtype(K_cache.dtype),
                                   **_descale_views(k_descale, v_descale, Q, B, H_kv), causal=causal, scale=scale,
                                   window=window, num_splits=n, workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
        return O, L
    if K_cache.dtype in FP8_CACHE_DTYPES:
        _lib.fa2_fwd_kvcache_fp8(Q, K_cache, V_cache, O, L, cache_seqlens, dtype, convert_triton_dtype(K_cache.dtype),
                                 **_descale_views(k_descale, v_descale, Q, B, H_kv), causal=causal, scale=scale,
                                 window=window, num_splits=n, workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
        return O, L
    _lib.fa2_fwd_kvcache(Q, K_cache, V_cache, O, L, cache_seqlens, dtype, causal=causal, scale=scale, window=window, num_splits=n,
                         workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
    return O, L


def _kvcache_mla_forward(Q, K_cache, V_cache, cache_seqlens, dev, causal, scale, window, num_splits, variant, k_descale, v_descale,
                         block_table, k_new, v_new, rotary_cos, rotary_sin, latent=False, kv_descale=None, append=None):
    """flash_attention_kvcache_forward with a V_cache whose last axis differs from K_cache's (fa2_fwd_kvcache_mla), and -- latent:
    flash_attention_mla_decode_forward alone -- an fp8 cache with its one descale (fa2_fwd_kvcache_mla_fp8) and the fused step
    (fa2_fwd_kvcache_mla_append): `append` is its checked (c_new, pe_new, rotary_cos, rotary_sin, rotary_interleaved)."""
    fp8 = K_cache.dtype in FP8_CACHE_DTYPES or V_cache.dtype in FP8_CACHE_DTYPES
    if fp8 and not latent:
        raise ValueError(f"kvcache: an fp8 K_cache / V_cache ({K_cache.dtype}) is not supported with d_v != d here: "
                         f"flash_attention_mla_decode_forward takes an fp8 latent cache (kv_descale)")
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale), ("k_new", k_new), ("v_new", v_new), ("rotary_cos", rotary_cos),
                    ("rotary_sin", rotary_sin)):
        if t is not None:
            raise ValueError(f"kvcache: {name} is not supported with d_v != d (V_cache {tuple(V_cache.shape)} under K_cache "
                             f"{tuple(K_cache.shape)})" + (": flash_attention_mla_decode_forward takes an fp8 latent cache "
                                                           "(kv_descale)" if name.endswith("descale") else ""))
    check_kvcache_args(Q, K_cache, K_cache, cache_seqlens, window, num_splits, None, None, block_table)
    if V_cache.dtype != K_cache.dtype:
        raise ValueError("kvcache: K_cache and V_cache must have the same dtype")
    if kv_descale is not None and not fp8:
        raise ValueError(f"mla decode: kv_descale goes with an fp8 KV_cache, not with {K_cache.dtype}")
    kv_descale = _kvcache_descale("kv_descale", kv_descale, Q, Q.shape[0], K_cache.shape[1])
    d, d_v = K_cache.shape[3], V_cache.shape[3]
    if not 1 <= d <= 576 or not 1 <= d_v <= 512:
        raise ValueError(f"kvcache: with d_v != d, d must be in [1, 576] and d_v in [1, 512], got d = {d}, d_v = {d_v}")
    if variant not in _lib.KVCACHE_MLA_VARIANTS:
        raise ValueError(f"kvcache: with d_v != d, variant must be one of {sorted(_lib.KVCACHE_MLA_VARIANTS)}, got {variant!r}")
    _check_dev(dev, Q, K_cache, V_cache)
    B, H, N_q, _ = Q.shape
    H_kv = K_cache.shape[1]
    dtype = convert_triton_dtype(Q.dtype)
    n = num_splits or _lib.kvcache_mla_num_splits(B, H, H_kv, N_q, _capacity(K_cache, block_table), d, d_v, dtype)
    O, L, ws = _kvcache_outputs(Q, (B, H, N_q, d_v), (B, H, N_q), _lib.kvcache_workspace_bytes(B, H, N_q, d_v, n) if n > 1 else 0)
    if append is not None:
        c_new, pe_new, cos, sin, interleaved = append
        if c_new.shape[0] != B or c_new.device != Q.device:
            raise ValueError(f"mla decode: kv_new must have Q's batch size {B} and device ({Q.device}), got {tuple(c_new.shape)} on "
                             f"{c_new.device}")
        _lib.fa2_fwd_kvcache_mla_append(Q, K_cache, O, L, c_new, pe_new, cache_seqlens, torch.empty_like(cache_seqlens), dtype,
                                        convert_triton_dtype(K_cache.dtype), block_table=block_table, kv_descale=kv_descale,
                                        rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved,
                                        q_rot=None if cos is None else torch.empty(B, H, N_q, d, dtype=Q.dtype, device=Q.device),
                                        causal=causal, scale=scale, window=window, num_splits=n, workspace=ws,
                                        variant=_lib.KVCACHE_MLA_VARIANTS[variant])
        return O, L
    if fp8:  # the one descale of the shared row is K's and V's
        _lib.fa2_fwd_kvcache_mla_fp8(Q, K_cache, V_cache, O, L, cache_seqlens, dtype, convert_triton_dtype(K_cache.dtype),
                                     k_descale=kv_descale, v_descale=kv_descale, block_table=block_table, causal=causal, scale=scale,
                                     window=window, num_splits=n, workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
        return O, L
    _lib.fa2_fwd_kvcache_mla(Q, K_cache, V_cache, O, L, cache_seqlens, dtype, block_table=block_table, causal=causal, scale=scale,
                             window=window, num_splits=n, workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
    return O, L


def flash_attention_mla_decode_forward(Q, KV_cache, cache_seqlens, dev, *, d_v=512, causal=False, scale=1.0, window=None, num_splits=0,
                                       variant="auto", block_table=None, kv_descale=None, kv_new=None, rotary_cos=None, rotary_sin=None,
                                       rotary_interleaved=False):
    """Multi-head latent attention decode, absorbed form, over the shared latent cache (fa2_fwd_kvcache_mla) -> (O, L).  Q
    (B, H, N_q, d); KV_cache (B, H_kv, S_k, d) or, with block_table, the page pool (num_blocks, H_kv, page_size, d): one row per key,
    d_v latent columns followed by the rotary ones (DeepSeek-V2 / V3 / R1, Kimi: H_kv = 1, d = 576, d_v = 512).  The score takes all
    d columns, the value is the first d_v of the same row: with a cache in Q's dtype the call is flash_attention_kvcache_forward(Q,
    KV_cache, KV_cache[..., :d_v], ...) bit for bit, and every other argument is that function's.  O (B, H, N_q, d_v) and L
    (B, H, N_q) in Q's dtype.  1 <= d_v < d.

    fp8 latent cache (fa2_fwd_kvcache_mla_fp8): KV_cache in torch.float8_e4m3fn or torch.float8_e5m2 under float16 / bfloat16 Q,
    contiguous or a page pool; the row is kv_descale * float(KV_cache), kv_descale a float32 tensor on Q's device that broadcasts to
    (B, H_kv) (None: 1; finite and > 0) -- the one descale of the shared row, K's and V's alike; quantize_kv_cache(KV, dtype) makes
    both.  Only the storage is fp8: the bytes are converted exactly while they are staged, the arithmetic stays 16-bit, and with
    kv_descale None the result is, bit for bit, that of the cache converted to Q's dtype.  variant "mla16" then needs every stride
    of the cache a multiple of 16 elements.  kv_descale with a cache in Q's dtype is a ValueError.

    Append (fa2_fwd_kvcache_mla_append): with kv_new -- one tensor (B, H_kv, N_new, d) in Q's dtype, or the pair (c_new, pe_new)
    with last axes d_v and d - d_v, any strides -- the call first writes the new rows into KV_cache IN PLACE as mla_kvcache_append
    does, at key indices cache_seqlens[b] + t, and then attends over cache_seqlens + N_new keys (at most the capacity: tokens past it
    are dropped).  cache_seqlens is required, holds the lengths before the append and is not modified.  rotary_cos, rotary_sin
    (S_rot, rotary_dim / 2) in Q's dtype with unit last stride, rotary_dim <= d - d_v, rotate the columns [d_v, d_v + rotary_dim) of
    the new rows at cache_seqlens[b] + t and of Q (a copy: Q itself is not modified) at cache_seqlens[b] + i for row i when the call
    is causal or windowed, every row at cache_seqlens[b] otherwise, as flash-attn does; apply_rotary on those columns is the
    arithmetic, bit for bit.  They need kv_new.  Without kv_new the cache is only read.  Packed (ragged) queries over the same cache:
    flash_attention_mla_varlen_decode_forward."""
    if not isinstance(KV_cache, torch.Tensor) or KV_cache.dim() != 4:
        raise ValueError("mla decode: KV_cache must be a tensor (B, H_kv, S_k, d) or a pool (num_blocks, H_kv, page_size, d)")
    if isinstance(d_v, bool) or not isinstance(d_v, int) or not 1 <= d_v < KV_cache.shape[3]:
        raise ValueError(f"mla decode: d_v must be an int in [1, d - 1] = [1, {KV_cache.shape[3] - 1}], got {d_v!r}")
    append = None
    if kv_new is not None or rotary_cos is not None or rotary_sin is not None:
        check_mla_append_args(KV_cache, kv_new, cache_seqlens, d_v, kv_descale, block_table, rotary_cos, rotary_sin, Q)
        append = (*_mla_sources(kv_new, d_v), rotary_cos, rotary_sin, rotary_interleaved)
    return _kvcache_mla_forward(Q, KV_cache, KV_cache[..., :d_v], cache_seqlens, dev, causal, scale, window, num_splits, variant, None,
                                None, block_table, None, None, None, None, latent=True, kv_descale=kv_descale, append=append)


def _mla_sources(kv_new, d_v):
    """(c_new, pe_new) of a kv_new argument: the pair as it is, or the two views of the one tensor."""
    if isinstance(kv_new, torch.Tensor):
        return kv_new[..., :d_v], kv_new[..., d_v:]
    if isinstance(kv_new, (tuple, list)) and len(kv_new) == 2 and all(isinstance(t, torch.Tensor) for t in kv_new):
        return kv_new[0], kv_new[1]
    raise ValueError("mla: kv_new must be one tensor (..., d) or a pair (c_new, pe_new) of tensors")


def check_mla_append_args(KV_cache, kv_new, cache_seqlens, d_v=512, kv_descale=None, block_table=None, rotary_cos=None, rotary_sin=None,
                          Q=None, cu_seqlens_new=None, max_seqlen_new=None):
    """ValueError for what mla_kvcache_append, mla_kvcache_append_varlen (with cu_seqlens_new and max_seqlen_new: kv_new packed) and
    the append keywords of flash_attention_mla_decode_forward (with Q, which is rotated along) cannot take.  Pure: takes CPU tensors
    as well."""
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError("mla: rotary_cos and rotary_sin go together")
    if kv_new is None:
        if rotary_cos is not None:
            raise ValueError("mla: rotary_cos / rotary_sin need kv_new (the rotation is part of the cache update)")
        return
    if cache_seqlens is None:
        raise ValueError("mla: kv_new needs cache_seqlens (the position the new tokens go to)")
    if not isinstance(KV_cache, torch.Tensor) or KV_cache.dim() != 4 or not 2 <= KV_cache.shape[3] <= 576:
        raise ValueError("mla: KV_cache must be a tensor (B, H_kv, S_k, d) or a pool (num_blocks, H_kv, page_size, d) with d in [2, 576]")
    d = KV_cache.shape[3]
    if isinstance(d_v, bool) or not isinstance(d_v, int) or not 1 <= d_v < d:
        raise ValueError(f"mla: d_v must be an int in [1, d - 1] = [1, {d - 1}], got {d_v!r}")
    c_new, pe_new = _mla_sources(kv_new, d_v)
    packed = cu_seqlens_new is not None or max_seqlen_new is not None
    lead = 2 if packed else 3  # the axes in front of the columns
    if c_new.dim() != lead + 1 or c_new.shape[:lead] != pe_new.shape[:lead] or c_new.shape[lead] != d_v or pe_new.shape[lead] != d - d_v \
            or c_new.shape[lead - 1 if packed else 1] != KV_cache.shape[1] or c_new.shape[0 if packed else 2] < 1 \
            or (not packed and block_table is None and c_new.shape[0] != KV_cache.shape[0]):
        raise ValueError(f"mla: kv_new must be {'packed (total_new, H_kv, d)' if packed else '(B, H_kv, N_new, d)'} or a pair with last "
                         f"axes d_v = {d_v} and d - d_v = {d - d_v}, at least one token, B, H_kv and d = {d} the cache's: got "
                         f"{tuple(c_new.shape)} and {tuple(pe_new.shape)} beside KV_cache {tuple(KV_cache.shape)}")
    if c_new.dtype != pe_new.dtype:
        raise ValueError("mla: both tensors of kv_new must have the same dtype")
    if c_new.dtype in FP8_CACHE_DTYPES:
        raise ValueError(f"mla: dtype {c_new.dtype} is not supported for kv_new (an fp8 cache takes float16 / bfloat16)")
    if packed:
        if not isinstance(cu_seqlens_new, torch.Tensor) or cu_seqlens_new.dtype != torch.int32 or cu_seqlens_new.dim() != 1 \
                or not cu_seqlens_new.is_contiguous() or cu_seqlens_new.numel() < 2:
            raise ValueError("mla: cu_seqlens_new must be a contiguous int32 tensor of B + 1 >= 2 entries")
        if cu_seqlens_new.device != c_new.device:
            raise ValueError(f"mla: cu_seqlens_new must be on kv_new's device ({c_new.device}), got {cu_seqlens_new.device}")
        if isinstance(max_seqlen_new, bool) or not isinstance(max_seqlen_new, int) or not 1 <= max_seqlen_new <= 1 << 28:
            raise ValueError(f"mla: max_seqlen_new must be an int in [1, 2^28], got {max_seqlen_new!r}")
        if c_new.shape[0] > 1 << 28 or c_new.shape[0] * 2 * c_new.shape[1] > 1 << 40:
            raise ValueError(f"mla: total_new must be <= 2^28 and total_new * 2 * H_kv <= 2^40, got total_new = {c_new.shape[0]}")
    B, H_kv = (cu_seqlens_new.numel() - 1, c_new.shape[1]) if packed else c_new.shape[:2]
    if KV_cache.dtype in FP8_CACHE_DTYPES:
        if c_new.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"mla: an fp8 cache needs kv_new in float16 or bfloat16, got {c_new.dtype}")
        _kvcache_descale("kv_descale", kv_descale, c_new, B, H_kv)
    else:
        if c_new.dtype != KV_cache.dtype:
            raise ValueError("mla: kv_new must have the cache's dtype (or the cache an fp8 dtype under 16-bit kv_new)")
        if kv_descale is not None:
            raise ValueError(f"mla: kv_descale goes with an fp8 KV_cache, not with {KV_cache.dtype}")
    convert_triton_dtype(c_new.dtype)
    if Q is not None and (packed or not isinstance(Q, torch.Tensor) or Q.dim() != 4 or Q.shape[3] != d or Q.dtype != c_new.dtype
                          or Q.shape[0] != c_new.shape[0]):
        raise ValueError(f"mla: Q goes with the fixed form and must be (B, H, N_q, d) in kv_new's dtype with its B and d = {d}")
    for name, t in (("kv_new[1]", pe_new), ("KV_cache", KV_cache)):
        if t.device != c_new.device:
            raise ValueError(f"mla: {name} must be on kv_new's device ({c_new.device}), got {t.device}")
    _check_cache_seqlens(cache_seqlens, B, c_new, "kv_new")
    if block_table is not None:
        _check_block_table(block_table, B, KV_cache.shape[2], c_new, "kv_new")
    if rotary_cos is not None:
        _check_rotary_tables(rotary_cos, rotary_sin, d - d_v, f"d - d_v = {d - d_v}", c_new, "kv_new")


def mla_kvcache_append(KV_cache, kv_new, cache_seqlens, *, d_v=512, kv_descale=None, block_table=None, rotary_cos=None, rotary_sin=None,
                       rotary_interleaved=False):
    """The cache update of an MLA decode step alone (include/fa2_fwd.h fa2_kvcache_mla_append) -> new_seqlens, int32 (B,): what an
    engine passes as the next step's cache_seqlens.  KV_cache is flash_attention_mla_decode_forward's latent cache, contiguous or a
    pool with block_table, in kv_new's dtype or fp8 with its one kv_descale.  kv_new: one tensor (B, H_kv, N_new, d), or the pair
    (c_new, pe_new) an engine holds -- the normalised latent (B, H_kv, N_new, d_v) and the un-rotated positional part
    (B, H_kv, N_new, d - d_v) -- any strides.  Token t of sequence b becomes the row at key index clamp(cache_seqlens[b], 0, capacity)
    + t, written IN PLACE: columns [0, d_v) from c_new, [d_v, d) from pe_new with its first rotary_dim columns rotated at that
    position by rotary_cos / rotary_sin (apply_rotary on pe_new is the arithmetic; rotary_dim <= d - d_v), the whole row quantised
    with kv_descale where the cache is fp8.  Tokens past the capacity are dropped and new_seqlens = min(cache_seqlens + N_new,
    capacity); cache_seqlens is not modified.  Everything else is kvcache_append's."""
    if kv_new is None:
        raise ValueError("mla: mla_kvcache_append needs kv_new")
    check_mla_append_args(KV_cache, kv_new, cache_seqlens, d_v, kv_descale, block_table, rotary_cos, rotary_sin)
    c_new, pe_new = _mla_sources(kv_new, d_v)
    new_seqlens = torch.empty_like(cache_seqlens)
    _lib.fa2_kvcache_mla_append(KV_cache, c_new, pe_new, cache_seqlens, new_seqlens, convert_triton_dtype(c_new.dtype),
                                convert_triton_dtype(KV_cache.dtype), block_table=block_table,
                                kv_descale=_kvcache_descale("kv_descale", kv_descale, c_new, *c_new.shape[:2]), rotary_cos=rotary_cos,
                                rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved)
    return new_seqlens


def mla_kvcache_append_varlen(KV_cache, kv_new, cu_seqlens_new, max_seqlen_new, cache_seqlens, *, d_v=512, kv_descale=None,
                              block_table=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False):
    """mla_kvcache_append for a ragged batch in one launch (include/fa2_fwd.h fa2_kvcache_mla_append_varlen) -> new_seqlens, int32
    (B,).  kv_new packed: one tensor (total_new, H_kv, d) or the pair (total_new, H_kv, d_v), (total_new, H_kv, d - d_v), any strides;
    cu_seqlens_new and max_seqlen_new as in kvcache_append_varlen: sequence b brings the min(cu[b + 1] - cu[b], max_seqlen_new) rows
    from cu[b] on, none is legal, rows outside every sequence are not read, and new_seqlens is written for every sequence."""
    if kv_new is None:
        raise ValueError("mla: mla_kvcache_append_varlen needs kv_new")
    check_mla_append_args(KV_cache, kv_new, cache_seqlens, d_v, kv_descale, block_table, rotary_cos, rotary_sin,
                          cu_seqlens_new=cu_seqlens_new, max_seqlen_new=max_seqlen_new)
    c_new, pe_new = _mla_sources(kv_new, d_v)
    new_seqlens = torch.empty_like(cache_seqlens)
    _lib.fa2_kvcache_mla_append_varlen(KV_cache, c_new, pe_new, cu_seqlens_new, max_seqlen_new, cache_seqlens, new_seqlens,
                                       convert_triton_dtype(c_new.dtype), convert_triton_dtype(KV_cache.dtype), block_table=block_table,
                                       kv_descale=_kvcache_descale("kv_descale", kv_descale, c_new, cu_seqlens_new.numel() - 1,
                                                                   c_new.shape[1]),
                                       rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved)
    return new_seqlens


def check_varlen_kvcache_args(Q, K_cache, V_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, window, num_splits, k_descale=None,
                              v_descale=None, block_table=None, k_new=None, v_new=None, rotary_cos=None, rotary_sin=None):
    """ValueError for what flash_attention_varlen_kvcache_forward cannot take (the packed Q and cu_seqlens_q, max_seqlen_q, and
    every rule of check_kvcache_args for the cache, its lengths, table, descales, window and num_splits; with the append keywords,
    every rule of check_kvcache_append_varlen_args).  Pure: takes CPU tensors as well."""
    if not isinstance(Q, torch.Tensor) or Q.dim() != 3 or Q.shape[0] < 1:
        raise ValueError(f"varlen kvcache: Q must be packed (total_q, H, d) with total_q >= 1, got "
                         f"{tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__}")
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 \
            or not cu_seqlens_q.is_contiguous() or cu_seqlens_q.numel() < 2:
        raise ValueError("varlen kvcache: cu_seqlens_q must be a contiguous int32 tensor of B + 1 >= 2 entries")
    if cu_seqlens_q.device != Q.device:
        raise ValueError(f"varlen kvcache: cu_seqlens_q must be on Q's device ({Q.device}), got {cu_seqlens_q.device}")
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or not 1 <= max_seqlen_q <= 1 << 28:
        raise ValueError(f"varlen kvcache: max_seqlen_q must be an int in [1, 2^28], got {max_seqlen_q!r}")
    if Q.shape[0] * Q.shape[1] > 1 << 40:
        raise ValueError(f"varlen kvcache: total_q * H must be <= 2^40, got {Q.shape[0]} * {Q.shape[1]}")
    B = cu_seqlens_q.numel() - 1
    # the cache's rules are the fixed-N_q call's: seen through a (B, H, 1, d) view of Q (no data is read)
    check_kvcache_args(Q[:1].transpose(0, 1).unsqueeze(0).expand(B, -1, -1, -1), K_cache, V_cache, cache_seqlens, window, num_splits,
                       k_descale, v_descale, block_table)
    if k_new is not None or v_new is not None or rotary_cos is not None or rotary_sin is not None:
        check_kvcache_append_varlen_args(K_cache, V_cache, k_new, v_new, cu_seqlens_q, max_seqlen_q, cache_seqlens, k_descale, v_descale,
                                         block_table, rotary_cos, rotary_sin, Q)
        if k_new.device != Q.device:
            raise ValueError(f"varlen kvcache: k_new, v_new must be on Q's device ({Q.device}), got {k_new.device}")


def flash_attention_varlen_kvcache_forward(Q, K_cache, V_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, dev, *, causal=False,
                                           scale=1.0, window=None, num_splits=0, variant="auto", k_descale=None, v_descale=None,
                                           block_table=None, k_new=None, v_new=None, rotary_cos=None, rotary_sin=None,
                                           rotary_interleaved=False):
    """Attention of variable-length (packed) queries over the KV cache (include/fa2_fwd.h fa2_fwd_kvcache_varlen) -> (O, L): what a
    chunked prefill, a mixed prefill / decode batch or the verification of draft tokens needs (flash-attn's
    flash_attn_varlen_func(..., block_table=)).  Q (total_q, H, d), any strides; cu_seqlens_q int32 (B + 1,) on Q's device:
    sequence b owns min(cu[b + 1] - cu[b], max_seqlen_q) rows from cu[b] on, none is legal.  K_cache, V_cache, cache_seqlens,
    k_descale, v_descale and block_table are flash_attention_kvcache_forward's: the contiguous (B, H_kv, S_k, d) cache or a page
    pool behind a block table, in Q's dtype or fp8.  The keys of the chunk's own tokens are already in the cache (kvcache_append puts
    them there), so query i of sequence b stands at position cache_seqlens[b] - n_q(b) + i: causal and window are bottom-right
    aligned per sequence.  O (total_q, H, d) contiguous, L (H, total_q) log2-domain, both in Q's dtype; rows without a visible key
    get O = 0, L = +inf; rows outside every sequence are not written (they hold what torch.empty left).  num_splits = 0 lets the
    library choose; variant is one of _lib.KVCACHE_VARIANTS ("mfma16": f16 / bf16, d 64 / 128, H / H_kv <= 64).  With every sequence
    at n_q = max_seqlen_q = N_q and (H / H_kv) * N_q <= 64 the result equals flash_attention_kvcache_forward's at the same explicit
    num_splits bit for bit.  No autograd, no autotuner.

    Append (fa2_fwd_kvcache_varlen_append): with k_new, v_new packed (total_q, H_kv, d) in Q's dtype on Q's device, any strides --
    token i of Q, k_new and v_new is the same token -- the call first updates K_cache / V_cache IN PLACE as kvcache_append_varlen
    does over cu_seqlens_q, and then attends over cache_seqlens + n_q(b) keys (at most the capacity).  cache_seqlens is required,
    holds the lengths BEFORE the append and is not modified.  rotary_cos, rotary_sin (S_rot, rotary_dim / 2) rotate K token t at
    position cache_seqlens[b] + t and Q (a copy) row i at cache_seqlens[b] + i when the call is causal or windowed, every row at
    cache_seqlens[b] otherwise: flash_attention_kvcache_forward's rule, which a uniform batch reproduces bit for bit.  They need
    k_new / v_new."""
    check_varlen_kvcache_args(Q, K_cache, V_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, window, num_splits, k_descale, v_descale,
                              block_table, k_new, v_new, rotary_cos, rotary_sin)
    if variant not in _lib.KVCACHE_VARIANTS:
        raise ValueError(f"varlen kvcache: variant must be one of {sorted(_lib.KVCACHE_VARIANTS)}, got {variant!r}")
    _check_dev(dev, Q, K_cache, V_cache)
    total_q, H, d = Q.shape
    B, H_kv = cu_seqlens_q.numel() - 1, K_cache.shape[1]
    dtype = convert_triton_dtype(Q.dtype)
    n = num_splits or _lib.kvcache_varlen_num_splits(B, H, H_kv, total_q, max_seqlen_q, _capacity(K_cache, block_table), d, dtype)
    O, L, ws = _kvcache_outputs(Q, (total_q, H, d), (H, total_q), _lib.kvcache_varlen_workspace_bytes(total_q, H, d, n) if n > 1 else 0)
    if k_new is not None:
        _lib.fa2_fwd_kvcache_varlen_append(Q, K_cache, V_cache, O, L, k_new, v_new, cu_seqlens_q, max_seqlen_q, cache_seqlens,
                                           torch.empty_like(cache_seqlens), dtype, convert_triton_dtype(K_cache.dtype),
                                           block_table=block_table, **_descale_views(k_descale, v_descale, Q, B, H_kv), rotary_cos=rotary_cos,
                                           rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved,
                                           q_rot=None if rotary_cos is None else torch.empty(total_q, H, d, dtype=Q.dtype, device=Q.device),
                                           causal=causal, scale=scale, window=window, num_splits=n, workspace=ws,
                                           variant=_lib.KVCACHE_VARIANTS[variant])
        return O, L
    _lib.fa2_fwd_kvcache_varlen(Q, K_cache, V_cache, O, L, cu_seqlens_q, max_seqlen_q, cache_seqlens, dtype,
                                convert_triton_dtype(K_cache.dtype), block_table=block_table,
                                **_descale_views(k_descale, v_descale, Q, B, H_kv), causal=causal, scale=scale,
                                window=window, num_splits=n, workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
    return O, L


def check_mla_varlen_args(Q, KV_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, d_v=512, window=None, num_splits=0, kv_descale=None,
                          block_table=None, kv_new=None, rotary_cos=None, rotary_sin=None):
    """ValueError for what flash_attention_mla_varlen_decode_forward cannot take: the packed Q, cu_seqlens_q and max_seqlen_q by the
    rules of check_varlen_kvcache_args, the latent cache, d_v, kv_descale, cache_seqlens, block_table, window and num_splits by those
    of flash_attention_mla_decode_forward, and with kv_new or the rotary tables every rule of check_mla_append_args for packed tokens
    over the same cu_seqlens_q.  Pure: takes CPU tensors as well."""
    if not isinstance(Q, torch.Tensor) or Q.dim() != 3 or Q.shape[0] < 1:
        raise ValueError(f"mla varlen decode: Q must be packed (total_q, H, d) with total_q >= 1, got "
                         f"{tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__}")
    if not isinstance(KV_cache, torch.Tensor) or KV_cache.dim() != 4:
        raise ValueError("mla varlen decode: KV_cache must be a tensor (B, H_kv, S_k, d) or a pool (num_blocks, H_kv, page_size, d)")
    d = KV_cache.shape[3]
    if isinstance(d_v, bool) or not isinstance(d_v, int) or not 1 <= d_v < d:
        raise ValueError(f"mla varlen decode: d_v must be an int in [1, d - 1] = [1, {d - 1}], got {d_v!r}")
    if not 1 <= d <= 576 or d_v > 512:
        raise ValueError(f"mla varlen decode: d must be in [1, 576] and d_v in [1, 512], got d = {d}, d_v = {d_v}")
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 \
            or not cu_seqlens_q.is_contiguous() or cu_seqlens_q.numel() < 2:
        raise ValueError("mla varlen decode: cu_seqlens_q must be a contiguous int32 tensor of B + 1 >= 2 entries")
    if cu_seqlens_q.device != Q.device:
        raise ValueError(f"mla varlen decode: cu_seqlens_q must be on Q's device ({Q.device}), got {cu_seqlens_q.device}")
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or not 1 <= max_seqlen_q <= 1 << 28:
        raise ValueError(f"mla varlen decode: max_seqlen_q must be an int in [1, 2^28], got {max_seqlen_q!r}")
    if Q.shape[0] * Q.shape[1] > 1 << 40:
        raise ValueError(f"mla varlen decode: total_q * H must be <= 2^40, got {Q.shape[0]} * {Q.shape[1]}")
    B = cu_seqlens_q.numel() - 1
    fp8 = KV_cache.dtype in FP8_CACHE_DTYPES
    if kv_descale is not None and not fp8:
        raise ValueError(f"mla varlen decode: kv_descale goes with an fp8 KV_cache, not with {KV_cache.dtype}")
    # the cache's rules are the fixed-N_q call's: seen through a (B, H, 1, d) view of Q (no data is read), K and V the one tensor
    check_kvcache_args(Q[:1].transpose(0, 1).unsqueeze(0).expand(B, -1, -1, -1), KV_cache, KV_cache, cache_seqlens, window, num_splits,
                       None, None, block_table)
    _kvcache_descale("kv_descale", kv_descale, Q, B, KV_cache.shape[1])
    if kv_new is not None or rotary_cos is not None or rotary_sin is not None:
        check_mla_append_args(KV_cache, kv_new, cache_seqlens, d_v, kv_descale, block_table, rotary_cos, rotary_sin,
                              cu_seqlens_new=cu_seqlens_q, max_seqlen_new=max_seqlen_q)
        c_new = _mla_sources(kv_new, d_v)[0]
        if c_new.shape[0] != Q.shape[0] or c_new.dtype != Q.dtype or c_new.device != Q.device:
            raise ValueError(f"mla varlen decode: kv_new must have Q's total_q = {Q.shape[0]}, dtype ({Q.dtype}) and device ({Q.device}), "
                             f"got {tuple(c_new.shape)} in {c_new.dtype} on {c_new.device}")


def flash_attention_mla_varlen_decode_forward(Q, KV_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, dev, *, d_v=512, causal=False,
                                              scale=1.0, window=None, num_splits=0, variant="auto", block_table=None, kv_descale=None,
                                              kv_new=None, rotary_cos=None, rotary_sin=None, rotary_interleaved=False):
    """Multi-head latent attention of variable-length (packed) queries over the shared latent cache (include/fa2_fwd.h
    fa2_fwd_kvcache_mla_varlen) -> (O, L): the verification of MTP / draft tokens, a mixed step of a prefill chunk beside one-token
    decodes, a prefix-cached chunk, in one call.  Q (total_q, H, d), any strides; cu_seqlens_q int32 (B + 1,) on Q's device and
    max_seqlen_q as in flash_attention_varlen_kvcache_forward: sequence b owns min(cu[b + 1] - cu[b], max_seqlen_q) rows from cu[b]
    on, none is legal, and query i of it stands at position cache_seqlens[b] - n_q(b) + i (causal and window bottom-right aligned per
    sequence).  KV_cache, d_v, cache_seqlens, block_table and kv_descale are flash_attention_mla_decode_forward's: the contiguous
    (B, H_kv, S_k, d) latent cache or a page pool, in Q's dtype or fp8 with its one descale.  O (total_q, H, d_v) contiguous, L
    (H, total_q) log2-domain, both in Q's dtype; rows without a visible key get O = 0, L = +inf; rows outside every sequence are not
    written.  num_splits = 0 lets the library choose; variant is one of _lib.KVCACHE_MLA_VARIANTS: "mla16" (f16 / bf16, d = 576,
    d_v = 512, unit d-stride and 16-byte aligned rows, contiguous or paged with page_size % 64 == 0, any H / H_kv), "generic"
    (everything else), "auto".  With every sequence at n_q = max_seqlen_q = N_q the result equals
    flash_attention_mla_decode_forward's at the same explicit num_splits bit for bit.  No autograd, no autotuner.

    Append (fa2_fwd_kvcache_mla_varlen_append): with kv_new -- one packed tensor (total_q, H_kv, d) in Q's dtype on Q's device, or the
    pair (c_new, pe_new) with last axes d_v and d - d_v, any strides, token i of Q and kv_new the same token -- the call first writes
    the new rows into KV_cache IN PLACE as mla_kvcache_append_varlen does over cu_seqlens_q, and then attends over cache_seqlens +
    n_q(b) keys (at most the capacity).  cache_seqlens is required, holds the lengths BEFORE the append and is not modified.
    rotary_cos, rotary_sin rotate the columns [d_v, d_v + rotary_dim) of new row t at cache_seqlens[b] + t and of Q (a copy) row i at
    cache_seqlens[b] + i when the call is causal or windowed, every row at cache_seqlens[b] otherwise:
    flash_attention_mla_decode_forward's rule.  They need kv_new."""
    check_mla_varlen_args(Q, KV_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, d_v, window, num_splits, kv_descale, block_table,
                          kv_new, rotary_cos, rotary_sin)
    if variant not in _lib.KVCACHE_MLA_VARIANTS:
        raise ValueError(f"mla varlen decode: variant must be one of {sorted(_lib.KVCACHE_MLA_VARIANTS)}, got {variant!r}")
    _check_dev(dev, Q, KV_cache, KV_cache)
    total_q, H, d = Q.shape
    B, H_kv = cu_seqlens_q.numel() - 1, KV_cache.shape[1]
    dtype = convert_triton_dtype(Q.dtype)
    n = num_splits or _lib.kvcache_mla_varlen_num_splits(B, H, H_kv, total_q, max_seqlen_q, _capacity(KV_cache, block_table), d, d_v, dtype)
    O, L, ws = _kvcache_outputs(Q, (total_q, H, d_v), (H, total_q), _lib.kvcache_varlen_workspace_bytes(total_q, H, d_v, n) if n > 1 else 0)
    kd = _kvcache_descale("kv_descale", kv_descale, Q, B, H_kv)
    if kv_new is not None:
        c_new, pe_new = _mla_sources(kv_new, d_v)
        _lib.fa2_fwd_kvcache_mla_varlen_append(Q, KV_cache, O, L, c_new, pe_new, cu_seqlens_q, max_seqlen_q, cache_seqlens,
                                               torch.empty_like(cache_seqlens), dtype, convert_triton_dtype(KV_cache.dtype),
                                               block_table=block_table, kv_descale=kd, rotary_cos=rotary_cos, rotary_sin=rotary_sin,
                                               rotary_interleaved=rotary_interleaved,
                                               q_rot=None if rotary_cos is None else torch.empty(total_q, H, d, dtype=Q.dtype, device=Q.device),
                                               causal=causal, scale=scale, window=window, num_splits=n, workspace=ws,
                                               variant=_lib.KVCACHE_MLA_VARIANTS[variant])
        return O, L
    _lib.fa2_fwd_kvcache_mla_varlen(Q, KV_cache, O, L, cu_seqlens_q, max_seqlen_q, cache_seqlens, dtype,
                                    convert_triton_dtype(KV_cache.dtype), d_v, block_table=block_table, kv_descale=kd, causal=causal,
                                    scale=scale, window=window, num_splits=n, workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
    return O, L


def _sparse_indices(indices, B, H_kv, N_q):
    """The (B, H_kv, N_q, topk) view of an indices argument: 4-D as it is, (B, N_q, topk) expanded over the KV heads without a copy."""
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32 or indices.dim() not in (3, 4):
        raise ValueError(f"mla sparse decode: indices must be an int32 tensor (B, H_kv, N_q, topk) or (B, N_q, topk), got "
                         f"{(tuple(indices.shape), indices.dtype) if isinstance(indices, torch.Tensor) else type(indices).__name__}")
    view = indices if indices.dim() == 4 else indices.unsqueeze(1).expand(-1, H_kv, -1, -1)
    if view.shape[:3] != (B, H_kv, N_q) or view.shape[3] < 1:
        raise ValueError(f"mla sparse decode: indices must be (B, H_kv, N_q, topk) = ({B}, {H_kv}, {N_q}, topk) or (B, N_q, topk) with "
                         f"topk >= 1, got {tuple(indices.shape)}")
    if view.shape[3] > 1 << 28:
        raise ValueError(f"mla sparse decode: topk must be <= 2^28, got {view.shape[3]}")
    if any(s < 0 for s in view.stride()):
        raise ValueError(f"mla sparse decode: indices with negative strides are not supported, got {tuple(view.stride())}")
    return view


def check_mla_sparse_args(Q, KV_cache, indices, cache_seqlens, d_v=512, num_splits=0, kv_descale=None, block_table=None):
    """ValueError for what flash_attention_mla_sparse_decode_forward cannot take: Q, the latent cache, d_v, cache_seqlens, block_table
    and num_splits by the rules of flash_attention_mla_decode_forward; indices int32 on Q's device, (B, H_kv, N_q, topk) or
    (B, N_q, topk) with B and N_q Q's and topk >= 1; kv_descale with a cache in Q's dtype, and an fp8 cache WITHOUT its kv_descale (a
    quantised cache has one: this call does not read None as 1).  Pure: takes CPU tensors as well."""
    if not isinstance(Q, torch.Tensor) or Q.dim() != 4:
        raise ValueError(f"mla sparse decode: Q must be a tensor (B, H, N_q, d), got "
                         f"{tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__}")
    if not isinstance(KV_cache, torch.Tensor) or KV_cache.dim() != 4:
        raise ValueError("mla sparse decode: KV_cache must be a tensor (B, H_kv, S_k, d) or a pool (num_blocks, H_kv, page_size, d)")
    d = KV_cache.shape[3]
    if isinstance(d_v, bool) or not isinstance(d_v, int) or not 1 <= d_v < d:
        raise ValueError(f"mla sparse decode: d_v must be an int in [1, d - 1] = [1, {d - 1}], got {d_v!r}")
    if not 1 <= d <= 576 or d_v > 512:
        raise ValueError(f"mla sparse decode: d must be in [1, 576] and d_v in [1, 512], got d = {d}, d_v = {d_v}")
    fp8 = KV_cache.dtype in FP8_CACHE_DTYPES
    if kv_descale is not None and not fp8:
        raise ValueError(f"mla sparse decode: kv_descale goes with an fp8 KV_cache, not with {KV_cache.dtype}")
    if fp8 and kv_descale is None:
        raise ValueError(f"mla sparse decode: an fp8 KV_cache ({KV_cache.dtype}) needs its kv_descale (quantize_kv_cache returns it)")
    check_kvcache_args(Q, KV_cache, KV_cache, cache_seqlens, None, num_splits, None, None, block_table)
    _kvcache_descale("kv_descale", kv_descale, Q, Q.shape[0], KV_cache.shape[1])
    view = _sparse_indices(indices, Q.shape[0], KV_cache.shape[1], Q.shape[2])
    if view.device != Q.device:
        raise ValueError(f"mla sparse decode: indices must be on Q's device ({Q.device}), got {view.device}")


def flash_attention_mla_sparse_decode_forward(Q, KV_cache, indices, cache_seqlens, dev, *, d_v=512, scale=1.0, num_splits=0,
                                              variant="auto", kv_descale=None, block_table=None, **mask):
    """Sparse multi-head latent attention over the shared latent cache (include/fa2_fwd.h fa2_fwd_kvcache_mla_sparse) -> (O, L): every
    (sequence, KV head, query position) attends over exactly the keys its list names (DeepSeek-V3.2's sparse attention: an indexer
    picks about 2,048 keys per query token, in decode and in a sparse prefill chunk alike).  No row is gathered: each listed row is
    read where it lies.  Q (B, H, N_q, d); KV_cache, d_v, cache_seqlens, block_table and kv_descale are
    flash_attention_mla_decode_forward's -- the contiguous (B, H_kv, S_k, d) latent cache or a page pool of ANY page size, in Q's dtype
    or fp8 with its kv_descale (required here).  indices: int32 on Q's device, (B, H_kv, N_q, topk), any non-negative strides, or
    (B, N_q, topk), expanded over the KV heads without a copy.  Entry [b, hk, qi, s] is a logical key position of sequence b; an entry
    < 0 or >= N_k(b) = clamp(cache_seqlens[b]) is no key (pad a shorter list with -1), a key listed twice counts twice, and a row
    without a valid entry gets O = 0, L = +inf.  The list is the mask: there is no causal and no window argument (both are a
    ValueError; the indexer respects causality).  O (B, H, N_q, d_v) contiguous, L (B, H, N_q) log2-domain, both in Q's dtype.
    num_splits = 0 lets the library choose (the splits run over the slots of the list); variant is one of _lib.KVCACHE_MLA_VARIANTS:
    "mla16" (f16 / bf16, d = 576, d_v = 512, unit d-stride and 16-byte aligned rows, any H / H_kv, any page size), "generic" (everything
    else), "auto".  The append side is mla_kvcache_append, called first.  No autograd, no autotuner."""
    for name in mask:
        if name in ("causal", "window"):
            raise ValueError(f"mla sparse decode: there is no {name} argument: the index list is the mask (the indexer respects "
                             f"causality; leave out what a position must not see)")
        raise TypeError(f"flash_attention_mla_sparse_decode_forward() got an unexpected keyword argument {name!r}")
    check_mla_sparse_args(Q, KV_cache, indices, cache_seqlens, d_v, num_splits, kv_descale, block_table)
    if variant not in _lib.KVCACHE_MLA_VARIANTS:
        raise ValueError(f"mla sparse decode: variant must be one of {sorted(_lib.KVCACHE_MLA_VARIANTS)}, got {variant!r}")
    _check_dev(dev, Q, KV_cache, KV_cache)
    B, H, N_q, d = Q.shape
    H_kv = KV_cache.shape[1]
    view = _sparse_indices(indices, B, H_kv, N_q)
    dtype = convert_triton_dtype(Q.dtype)
    n = num_splits or _lib.kvcache_mla_sparse_num_splits(B, H, H_kv, N_q, view.shape[3], d, d_v, dtype)
    O, L, ws = _kvcache_outputs(Q, (B, H, N_q, d_v), (B, H, N_q), _lib.kvcache_workspace_bytes(B, H, N_q, d_v, n) if n > 1 else 0)
    kd = _kvcache_descale("kv_descale", kv_descale, Q, B, H_kv)
    _lib.fa2_fwd_kvcache_mla_sparse(Q, KV_cache, KV_cache[..., :d_v], O, L, view, cache_seqlens, dtype, convert_triton_dtype(KV_cache.dtype),
                                    k_descale=kd, v_descale=kd, block_table=block_table, scale=scale, num_splits=n, workspace=ws,
                                    variant=_lib.KVCACHE_MLA_VARIANTS[variant])
    return O, L


INDEXER_Q_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def quantize_index_keys(k, dtype):
    """(k8, k_scale) of index keys (..., d_I) for the indexer's fp8 cache: one POWER-OF-TWO scale per row, the smallest with
    amax(row) / scale <= finfo(dtype).max (1 for a row of zeros), float32 of shape k.shape[:-1]; k8 = (k / scale) in dtype
    (torch.float8_e4m3fn or torch.float8_e5m2).  The division is exact, so k8.float() * k_scale[..., None] is exact in fp32 as
    well.  Plain torch, any device."""
    if dtype not in FP8_CACHE_DTYPES:
        raise ValueError(f"quantize_index_keys: dtype must be torch.float8_e4m3fn or torch.float8_e5m2, got {dtype}")
    if not isinstance(k, torch.Tensor) or k.dim() < 1 or not k.dtype.is_floating_point:
        raise ValueError("quantize_index_keys: k must be a floating-point tensor (..., d_I)")
    top = torch.finfo(dtype).max
    amax = k.detach().abs().amax(dim=-1).to(torch.float32)
    m, e = torch.frexp(amax / top)  # amax / top = m 2^e, m in [0.5, 1): ceil(log2) is e, or e - 1 at m = 0.5
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e - (m == 0.5).to(e.dtype)), torch.ones_like(amax))
    k8 = (k.to(torch.float32) / scale[..., None]).clamp(-top, top).to(dtype)
    return k8, scale


def _indexer_capacity(k_idx, block_table):
    return k_idx.shape[1] if block_table is None else block_table.shape[1] * k_idx.shape[1]


def check_mla_indexer_args(q_idx, weights, k_idx, cache_seqlens, topk=2048, k_scale=None, block_table=None):
    """ValueError, naming the argument, for what flash_attention_mla_indexer_topk cannot take: q_idx (B, H_I, N_q, d_I) in f16, bf16
    or f32 with d_I <= 576; weights float32 (B, H_I, N_q); k_idx (B, S_k, d_I), or the pool (num_blocks, page_size, d_I) with an int32
    block_table (B, max_blocks), in q_idx's dtype or fp8 under f16 / bf16; k_scale float32 shaped like k_idx's rows, required with an
    fp8 k_idx; cache_seqlens int32 (B,) or None; topk an int in [1, 2^28]; everything on q_idx's device.  Pure: takes CPU tensors."""
    who = "mla indexer"
    if not isinstance(q_idx, torch.Tensor) or q_idx.dim() != 4:
        raise ValueError(f"{who}: q_idx must be a tensor (B, H_I, N_q, d_I), got "
                         f"{tuple(q_idx.shape) if isinstance(q_idx, torch.Tensor) else type(q_idx).__name__}")
    if q_idx.dtype not in INDEXER_Q_DTYPES:
        raise ValueError(f"{who}: q_idx must be float16, bfloat16 or float32, got {q_idx.dtype}")
    B, H_I, N_q, d_I = q_idx.shape
    if min(B, H_I, N_q) < 1 or not 1 <= d_I <= 576:
        raise ValueError(f"{who}: q_idx needs B, H_I, N_q >= 1 and d_I in [1, 576], got {tuple(q_idx.shape)}")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (B, H_I, N_q):
        raise ValueError(f"{who}: weights must be a float32 tensor (B, H_I, N_q) = ({B}, {H_I}, {N_q})")
    if not isinstance(k_idx, torch.Tensor) or k_idx.dim() != 3 or k_idx.shape[2] != d_I or k_idx.shape[1] < 1:
        raise ValueError(f"{who}: k_idx must be a tensor (B, S_k, d_I) or a pool (num_blocks, page_size, d_I) with d_I = {d_I}")
    fp8 = k_idx.dtype in FP8_CACHE_DTYPES
    if fp8 and q_idx.dtype == torch.float32:
        raise ValueError(f"{who}: an fp8 k_idx ({k_idx.dtype}) goes with float16 / bfloat16 q_idx, not float32")
    if not fp8 and k_idx.dtype != q_idx.dtype:
        raise ValueError(f"{who}: k_idx must have q_idx's dtype ({q_idx.dtype}) or an fp8 dtype, got {k_idx.dtype}")
    if block_table is None:
        if k_idx.shape[0] != B:
            raise ValueError(f"{who}: k_idx must be (B, S_k, d_I) with B = {B}, got {tuple(k_idx.shape)} (a pool needs its block_table)")
    else:
        _check_block_table(block_table, B, k_idx.shape[1], q_idx, "q_idx")
    if fp8 and k_scale is None:
        raise ValueError(f"{who}: an fp8 k_idx ({k_idx.dtype}) needs its k_scale (quantize_index_keys returns it)")
    if k_scale is not None and (not isinstance(k_scale, torch.Tensor) or k_scale.dtype != torch.float32
                                or tuple(k_scale.shape) != tuple(k_idx.shape[:2])):
        raise ValueError(f"{who}: k_scale must be a float32 tensor shaped like k_idx's rows {tuple(k_idx.shape[:2])}")
    if cache_seqlens is not None:
        _check_cache_seqlens(cache_seqlens, B, q_idx, "q_idx", " (or None)")
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= 1 << 28:
        raise ValueError(f"{who}: topk must be an int in [1, 2^28], got {topk!r}")
    if _indexer_capacity(k_idx, block_table) > 1 << 28:
        raise ValueError(f"{who}: the capacity must be <= 2^28")
    for name, t in (("weights", weights), ("k_idx", k_idx), ("k_scale", k_scale)):
        if t is not None and t.device != q_idx.device:
            raise ValueError(f"{who}: {name} must be on q_idx's device ({q_idx.device}), got {t.device}")
    for name, t in (("q_idx", q_idx), ("weights", weights), ("k_idx", k_idx), ("k_scale", k_scale)):
        if t is not None and any(s < 0 for s in t.stride()):
            raise ValueError(f"{who}: {name} with negative strides is not supported")


def _indexer_variant(variant):
    if variant not in _lib.INDEXER_VARIANTS:
        raise ValueError(f"mla indexer: variant must be one of {sorted(_lib.INDEXER_VARIANTS)}, got {variant!r}")
    return _lib.INDEXER_VARIANTS[variant]


def _indexer_dev(dev, q_idx):
    if q_idx.device != torch.device(dev):
        raise ValueError(f"dev={dev} is not the device of q_idx ({q_idx.device})")


def mla_indexer_logits(q_idx, weights, k_idx, cache_seqlens, dev, *, causal=True, k_scale=None, block_table=None, variant="auto"):
    """The index scores of the MLA indexer alone (include/fa2_fwd.h fa2_mla_indexer_logits) -> logits float32 (B, N_q, capacity):
    logits[b, qi, j] = k_scale[b, j] * sum_h weights[b, h, qi] * relu(q_idx[b, h, qi] . k_idx[b, j]) for the candidates j < n(b, qi)
    of query qi (position N_k(b) - N_q + qi; causal: keys 0 .. position, else all N_k(b)).  Entries at j >= n(b, qi) are NOT written:
    the buffer comes from torch.empty.  Arguments as flash_attention_mla_indexer_topk."""
    check_mla_indexer_args(q_idx, weights, k_idx, cache_seqlens, 1, k_scale, block_table)
    v = _indexer_variant(variant)
    _indexer_dev(dev, q_idx)
    B, _, N_q, _ = q_idx.shape
    logits = torch.empty((B, N_q, _indexer_capacity(k_idx, block_table)), dtype=torch.float32, device=q_idx.device)
    _lib.fa2_mla_indexer_logits(q_idx, weights, k_idx, k_scale, logits, cache_seqlens, convert_triton_dtype(q_idx.dtype),
                                convert_triton_dtype(k_idx.dtype), block_table=block_table, causal=causal, variant=v)
    return logits


def topk_indices(logits, cache_seqlens, topk, *, N_q=None, causal=True):
    """The selection of the MLA indexer alone (fa2_topk_indices), over any float32 logits (B, N_q, S_k) of any non-negative strides
    (or (B * N_q, S_k) with N_q given) -> indices int32 (B, N_q, topk).  Row (b, qi) has n candidates, entries j < n with n as in
    mla_indexer_logits; nothing else of the row is read.  Its list is the min(topk, n) candidates first under (value descending,
    position ascending) -- -0.0 equals +0.0, a NaN ranks as -inf -- emitted in ascending position, the rest of the row -1."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() not in (2, 3):
        raise ValueError("topk indices: logits must be a float32 tensor (B, N_q, S_k)")
    if logits.dim() == 2:
        if isinstance(N_q, bool) or not isinstance(N_q, int) or N_q < 1 or logits.shape[0] % N_q:
            raise ValueError(f"topk indices: two-dimensional logits (B * N_q, S_k) need N_q, an int >= 1 dividing {logits.shape[0]}, got {N_q!r}")
        logits = logits.unflatten(0, (logits.shape[0] // N_q, N_q))
    elif N_q is not None and N_q != logits.shape[1]:
        raise ValueError(f"topk indices: N_q = {N_q!r} is not the logits' ({logits.shape[1]})")
    B, nq, S_k = logits.shape
    if min(B, nq, S_k) < 1 or S_k > 1 << 28 or any(s < 0 for s in logits.stride()):
        raise ValueError(f"topk indices: logits must be (B, N_q, S_k) with every size >= 1, S_k <= 2^28 and no negative stride, got "
                         f"{tuple(logits.shape)}, strides {tuple(logits.stride())}")
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= 1 << 28:
        raise ValueError(f"topk indices: topk must be an int in [1, 2^28], got {topk!r}")
    if cache_seqlens is not None:
        _check_cache_seqlens(cache_seqlens, B, logits, "logits", " (or None)")
    indices = torch.empty((B, nq, topk), dtype=torch.int32, device=logits.device)
    _lib.fa2_topk_indices(logits, indices, cache_seqlens, causal=causal)
    return indices


def flash_attention_mla_indexer_topk(q_idx, weights, k_idx, cache_seqlens, dev, topk=2048, causal=True, k_scale=None, block_table=None,
                                     variant="auto", return_logits=False):
    """The MLA indexer (DeepSeek-V3.2's lightning indexer; include/fa2_fwd.h fa2_mla_indexer_topk) -> indices int32 (B, N_q, topk),
    the key lists flash_attention_mla_sparse_decode_forward takes: scores and selection on one stream, no (B, N_q, H_I, N_k)
    intermediate.  q_idx (B, H_I, N_q, d_I) in f16, bf16 or f32, any strides; weights float32 (B, H_I, N_q), any softmax or head
    scale already folded in; k_idx the index-key cache (B, S_k, d_I) -- one shared head -- or, with block_table (B, max_blocks)
    int32, the pool (num_blocks, page_size, d_I) of ANY page size, in q_idx's dtype or fp8 under f16 / bf16 with k_scale (float32,
    shaped like the rows, > 0; quantize_index_keys makes both); cache_seqlens int32 (B,) or None (= the capacity).  Query qi of
    sequence b stands at position N_k(b) - N_q + qi; causal: its candidates are the keys up to that position, else all N_k(b).
    The list holds the min(topk, n) candidates of highest score (ties: the lower position), in ASCENDING position, padded with -1.
    variant is one of _lib.INDEXER_VARIANTS: "idx16" (f16 / bf16, d_I = 128, H_I <= 64, unit column strides, 16-byte aligned
    rows), "generic" (everything else), "auto".  return_logits: (indices, logits), the float32 (B, N_q, capacity) scores, written
    for the candidates only.  No autograd."""
    check_mla_indexer_args(q_idx, weights, k_idx, cache_seqlens, topk, k_scale, block_table)
    v = _indexer_variant(variant)
    _indexer_dev(dev, q_idx)
    B, _, N_q, _ = q_idx.shape
    logits = torch.empty((B, N_q, _indexer_capacity(k_idx, block_table)), dtype=torch.float32, device=q_idx.device)
    indices = torch.empty((B, N_q, topk), dtype=torch.int32, device=q_idx.device)
    _lib.fa2_mla_indexer_topk(q_idx, weights, k_idx, k_scale, logits, indices, cache_seqlens, convert_triton_dtype(q_idx.dtype),
                              convert_triton_dtype(k_idx.dtype), block_table=block_table, causal=causal, variant=v)
    return (indices, logits) if return_logits else indices


def _check_cu_seqlens_q(who, cu_seqlens_q, max_seqlen_q, anchor, anchor_name):
    """cu_seqlens_q and max_seqlen_q of a packed call, by the rules of check_mla_varlen_args; returns B."""
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 \
            or not cu_seqlens_q.is_contiguous() or cu_seqlens_q.numel() < 2:
        raise ValueError(f"{who}: cu_seqlens_q must be a contiguous int32 tensor of B + 1 >= 2 entries")
    if cu_seqlens_q.device != anchor.device:
        raise ValueError(f"{who}: cu_seqlens_q must be on {anchor_name}'s device ({anchor.device}), got {cu_seqlens_q.device}")
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or not 1 <= max_seqlen_q <= 1 << 28:
        raise ValueError(f"{who}: max_seqlen_q must be an int in [1, 2^28], got {max_seqlen_q!r}")
    return cu_seqlens_q.numel() - 1


def _sparse_varlen_indices(indices, total_q, H_kv):
    """The (total_q, H_kv, topk) view of a packed indices argument: 3-D as it is, (total_q, topk) expanded over the KV heads without a
    copy."""
    who = "mla sparse varlen decode"
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32 or indices.dim() not in (2, 3):
        raise ValueError(f"{who}: indices must be an int32 tensor (total_q, H_kv, topk) or (total_q, topk), got "
                         f"{(tuple(indices.shape), indices.dtype) if isinstance(indices, torch.Tensor) else type(indices).__name__}")
    view = indices if indices.dim() == 3 else indices.unsqueeze(1).expand(-1, H_kv, -1)
    if view.shape[:2] != (total_q, H_kv) or view.shape[2] < 1:
        raise ValueError(f"{who}: indices must be (total_q, H_kv, topk) = ({total_q}, {H_kv}, topk) or (total_q, topk) with topk >= 1, "
                         f"got {tuple(indices.shape)}")
    if view.shape[2] > 1 << 28:
        raise ValueError(f"{who}: topk must be <= 2^28, got {view.shape[2]}")
    if any(s < 0 for s in view.stride()):
        raise ValueError(f"{who}: indices with negative strides are not supported, got {tuple(view.stride())}")
    return view


def check_mla_sparse_varlen_args(Q, KV_cache, indices, cu_seqlens_q, max_seqlen_q, cache_seqlens, d_v=512, num_splits=0, kv_descale=None,
                                 block_table=None):
    """ValueError for what flash_attention_mla_sparse_varlen_decode_forward cannot take: the packed Q, cu_seqlens_q and max_seqlen_q by
    the rules of check_mla_varlen_args; the latent cache, d_v, cache_seqlens, block_table, num_splits and kv_descale by those of
    check_mla_sparse_args (an fp8 cache needs its kv_descale); indices int32 on Q's device, (total_q, H_kv, topk) or (total_q, topk)
    with topk >= 1.  Pure: takes CPU tensors as well."""
    who = "mla sparse varlen decode"
    if not isinstance(Q, torch.Tensor) or Q.dim() != 3 or Q.shape[0] < 1:
        raise ValueError(f"{who}: Q must be packed (total_q, H, d) with total_q >= 1, got "
                         f"{tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__}")
    if not isinstance(KV_cache, torch.Tensor) or KV_cache.dim() != 4:
        raise ValueError(f"{who}: KV_cache must be a tensor (B, H_kv, S_k, d) or a pool (num_blocks, H_kv, page_size, d)")
    d = KV_cache.shape[3]
    if isinstance(d_v, bool) or not isinstance(d_v, int) or not 1 <= d_v < d:
        raise ValueError(f"{who}: d_v must be an int in [1, d - 1] = [1, {d - 1}], got {d_v!r}")
    if not 1 <= d <= 576 or d_v > 512:
        raise ValueError(f"{who}: d must be in [1, 576] and d_v in [1, 512], got d = {d}, d_v = {d_v}")
    B = _check_cu_seqlens_q(who, cu_seqlens_q, max_seqlen_q, Q, "Q")
    if Q.shape[0] * Q.shape[1] > 1 << 40:
        raise ValueError(f"{who}: total_q * H must be <= 2^40, got {Q.shape[0]} * {Q.shape[1]}")
    fp8 = KV_cache.dtype in FP8_CACHE_DTYPES
    if kv_descale is not None and not fp8:
        raise ValueError(f"{who}: kv_descale goes with an fp8 KV_cache, not with {KV_cache.dtype}")
    if fp8 and kv_descale is None:
        raise ValueError(f"{who}: an fp8 KV_cache ({KV_cache.dtype}) needs its kv_descale (quantize_kv_cache returns it)")
    # the cache's rules are the fixed-N_q call's: seen through a (B, H, 1, d) view of Q (no data is read), K and V the one tensor
    check_kvcache_args(Q[:1].transpose(0, 1).unsqueeze(0).expand(B, -1, -1, -1), KV_cache, KV_cache, cache_seqlens, None, num_splits,
                       None, None, block_table)
    _kvcache_descale("kv_descale", kv_descale, Q, B, KV_cache.shape[1])
    view = _sparse_varlen_indices(indices, Q.shape[0], KV_cache.shape[1])
    if view.device != Q.device:
        raise ValueError(f"{who}: indices must be on Q's device ({Q.device}), got {view.device}")


def flash_attention_mla_sparse_varlen_decode_forward(Q, KV_cache, indices, cu_seqlens_q, max_seqlen_q, cache_seqlens, dev, *, d_v=512,
                                                     scale=1.0, num_splits=0, variant="auto", kv_descale=None, block_table=None, **mask):
    """Sparse multi-head latent attention of variable-length (packed) queries (include/fa2_fwd.h fa2_fwd_kvcache_mla_sparse_varlen)
    -> (O, L): flash_attention_mla_sparse_decode_forward for a ragged step -- a prefill chunk beside one-token decodes, draft tokens
    of a different count per sequence -- in one call.  Q (total_q, H, d), any strides; cu_seqlens_q int32 (B + 1,) on Q's device and
    max_seqlen_q as in flash_attention_mla_varlen_decode_forward: sequence b owns min(cu[b + 1] - cu[b], max_seqlen_q) rows from cu[b]
    on, none is legal.  indices: int32 on Q's device, (total_q, H_kv, topk), any non-negative strides, or (total_q, topk) -- what
    flash_attention_mla_indexer_topk_varlen returns -- expanded over the KV heads without a copy.  Entry [t, hk, s] is a logical key
    position of THE SEQUENCE THAT OWNS packed row t; an entry < 0 or >= N_k(b) of that sequence is no key, a key listed twice counts
    twice, a row without a valid entry gets O = 0, L = +inf.  KV_cache, d_v, cache_seqlens, block_table and kv_descale are
    flash_attention_mla_sparse_decode_forward's; so are causal= and window= (both a ValueError: the list is the mask), num_splits and
    variant.  O (total_q, H, d_v) contiguous, L (H, total_q) log2-domain, both in Q's dtype; rows outside every sequence are not
    written.  Sequence b's rows equal flash_attention_mla_sparse_decode_forward's on that sequence alone, bit for bit at the same
    explicit num_splits.  The append side is mla_kvcache_append_varlen, called first.  No autograd, no autotuner."""
    for name in mask:
        if name in ("causal", "window"):
            raise ValueError(f"mla sparse varlen decode: there is no {name} argument: the index list is the mask (the indexer respects "
                             f"causality; leave out what a position must not see)")
        raise TypeError(f"flash_attention_mla_sparse_varlen_decode_forward() got an unexpected keyword argument {name!r}")
    check_mla_sparse_varlen_args(Q, KV_cache, indices, cu_seqlens_q, max_seqlen_q, cache_seqlens, d_v, num_splits, kv_descale, block_table)
    if variant not in _lib.KVCACHE_MLA_VARIANTS:
        raise ValueError(f"mla sparse varlen decode: variant must be one of {sorted(_lib.KVCACHE_MLA_VARIANTS)}, got {variant!r}")
    _check_dev(dev, Q, KV_cache, KV_cache)
    total_q, H, d = Q.shape
    B, H_kv = cu_seqlens_q.numel() - 1, KV_cache.shape[1]
    view = _sparse_varlen_indices(indices, total_q, H_kv)
    dtype = convert_triton_dtype(Q.dtype)
    n = num_splits or _lib.kvcache_mla_sparse_varlen_num_splits(total_q, H, H_kv, view.shape[2], d, d_v, dtype)
    O, L, ws = _kvcache_outputs(Q, (total_q, H, d_v), (H, total_q), _lib.kvcache_varlen_workspace_bytes(total_q, H, d_v, n) if n > 1 else 0)
    kd = _kvcache_descale("kv_descale", kv_descale, Q, B, H_kv)
    _lib.fa2_fwd_kvcache_mla_sparse_varlen(Q, KV_cache, KV_cache[..., :d_v], O, L, view, cu_seqlens_q, max_seqlen_q, cache_seqlens, dtype,
                                           convert_triton_dtype(KV_cache.dtype), k_descale=kd, v_descale=kd, block_table=block_table,
                                           scale=scale, num_splits=n, workspace=ws, variant=_lib.KVCACHE_MLA_VARIANTS[variant])
    return O, L


def check_mla_indexer_varlen_args(q_idx, weights, k_idx, cu_seqlens_q, max_seqlen_q, cache_seqlens, topk=2048, k_scale=None,
                                  block_table=None):
    """ValueError, naming the argument, for what flash_attention_mla_indexer_topk_varlen cannot take: q_idx packed (total_q, H_I, d_I)
    and weights float32 (total_q, H_I); cu_seqlens_q and max_seqlen_q by the rules of check_mla_varlen_args; everything else by the
    rules of check_mla_indexer_args.  Pure: takes CPU tensors."""
    who = "mla indexer varlen"
    if not isinstance(q_idx, torch.Tensor) or q_idx.dim() != 3 or q_idx.shape[0] < 1:
        raise ValueError(f"{who}: q_idx must be packed (total_q, H_I, d_I) with total_q >= 1, got "
                         f"{tuple(q_idx.shape) if isinstance(q_idx, torch.Tensor) else type(q_idx).__name__}")
    total_q, H_I, _ = q_idx.shape
    if total_q > 1 << 28:
        raise ValueError(f"{who}: total_q must be <= 2^28, got {total_q}")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (total_q, H_I):
        raise ValueError(f"{who}: weights must be a float32 tensor (total_q, H_I) = ({total_q}, {H_I})")
    B = _check_cu_seqlens_q(who, cu_seqlens_q, max_seqlen_q, q_idx, "q_idx")
    # the key side's rules are the fixed call's: seen through (B, H_I, 1, d_I) / (B, H_I, 1) views of the first row (no data is read)
    check_mla_indexer_args(q_idx[:1].transpose(0, 1).unsqueeze(0).expand(B, -1, -1, -1), weights[:1].transpose(0, 1).unsqueeze(0).expand(B, -1, -1),
                           k_idx, cache_seqlens, topk, k_scale, block_table)
    for name, t in (("q_idx", q_idx), ("weights", weights)):
        if any(s < 0 for s in t.stride()):
            raise ValueError(f"{who}: {name} with negative strides is not supported")
    if weights.device != q_idx.device:
        raise ValueError(f"{who}: weights must be on q_idx's device ({q_idx.device}), got {weights.device}")


def mla_indexer_logits_varlen(q_idx, weights, k_idx, cu_seqlens_q, max_seqlen_q, cache_seqlens, dev, *, causal=True, k_scale=None,
                              block_table=None, variant="auto"):
    """The index scores of packed queries alone (include/fa2_fwd.h fa2_mla_indexer_logits_varlen) -> logits float32
    (total_q, capacity): row start(b) + i holds mla_indexer_logits' row of query i of sequence b, which stands at position
    N_k(b) - n_q(b) + i; entries at and past its candidate count, and rows no sequence owns, are NOT written: the buffer comes from
    torch.empty.  Arguments as flash_attention_mla_indexer_topk_varlen."""
    check_mla_indexer_varlen_args(q_idx, weights, k_idx, cu_seqlens_q, max_seqlen_q, cache_seqlens, 1, k_scale, block_table)
    v = _indexer_variant(variant)
    _indexer_dev(dev, q_idx)
    logits = torch.empty((q_idx.shape[0], _indexer_capacity(k_idx, block_table)), dtype=torch.float32, device=q_idx.device)
    _lib.fa2_mla_indexer_logits_varlen(q_idx, weights, k_idx, k_scale, logits, cu_seqlens_q, max_seqlen_q, cache_seqlens,
                                       convert_triton_dtype(q_idx.dtype), convert_triton_dtype(k_idx.dtype), block_table=block_table,
                                       causal=causal, variant=v)
    return logits


def topk_indices_varlen(logits, cu_seqlens_q, max_seqlen_q, cache_seqlens, topk, *, causal=True):
    """The selection of the MLA indexer over packed rows (fa2_topk_indices_varlen): float32 logits (total_q, S_k) of any non-negative
    strides -> indices int32 (total_q, topk).  Row start(b) + i is query i of sequence b and has topk_indices' candidates with n_q(b)
    in N_q's place; its list is topk_indices'.  A row no sequence owns is not written."""
    who = "topk indices varlen"
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError(f"{who}: logits must be a float32 tensor (total_q, S_k)")
    total_q, S_k = logits.shape
    if min(total_q, S_k) < 1 or max(total_q, S_k) > 1 << 28 or any(s < 0 for s in logits.stride()):
        raise ValueError(f"{who}: logits must be (total_q, S_k) with both sizes in [1, 2^28] and no negative stride, got "
                         f"{tuple(logits.shape)}, strides {tuple(logits.stride())}")
    B = _check_cu_seqlens_q(who, cu_seqlens_q, max_seqlen_q, logits, "logits")
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= 1 << 28:
        raise ValueError(f"{who}: topk must be an int in [1, 2^28], got {topk!r}")
    if cache_seqlens is not None:
        _check_cache_seqlens(cache_seqlens, B, logits, "logits", " (or None)")
    indices = torch.empty((total_q, topk), dtype=torch.int32, device=logits.device)
    _lib.fa2_topk_indices_varlen(logits, indices, cu_seqlens_q, max_seqlen_q, cache_seqlens, causal=causal)
    return indices


def flash_attention_mla_indexer_topk_varlen(q_idx, weights, k_idx, cu_seqlens_q, max_seqlen_q, cache_seqlens, dev, topk=2048, causal=True,
                                            k_scale=None, block_table=None, variant="auto", return_logits=False):
    """The MLA indexer over variable-length (packed) queries (include/fa2_fwd.h fa2_mla_indexer_topk_varlen) -> indices int32
    (total_q, topk), the key lists flash_attention_mla_sparse_varlen_decode_forward takes as they are.  q_idx (total_q, H_I, d_I) in
    f16, bf16 or f32, any strides; weights float32 (total_q, H_I); cu_seqlens_q int32 (B + 1,) on q_idx's device and max_seqlen_q as
    in flash_attention_mla_varlen_decode_forward; k_idx, k_scale, cache_seqlens, block_table, topk, causal, variant and return_logits
    are flash_attention_mla_indexer_topk's.  Query i of sequence b stands at position N_k(b) - n_q(b) + i.  Sequence b's rows equal
    flash_attention_mla_indexer_topk's on that sequence alone, byte for byte; rows no sequence owns are not written.  return_logits:
    (indices, logits), the float32 (total_q, capacity) scores.  No autograd."""
    check_mla_indexer_varlen_args(q_idx, weights, k_idx, cu_seqlens_q, max_seqlen_q, cache_seqlens, topk, k_scale, block_table)
    v = _indexer_variant(variant)
    _indexer_dev(dev, q_idx)
    total_q = q_idx.shape[0]
    logits = torch.empty((total_q, _indexer_capacity(k_idx, block_table)), dtype=torch.float32, device=q_idx.device)
    indices = torch.empty((total_q, topk), dtype=torch.int32, device=q_idx.device)
    _lib.fa2_mla_indexer_topk_varlen(q_idx, weights, k_idx, k_scale, logits, indices, cu_seqlens_q, max_seqlen_q, cache_seqlens,
                                     convert_triton_dtype(q_idx.dtype), convert_triton_dtype(k_idx.dtype), block_table=block_table,
                                     causal=causal, variant=v)
    return (indices, logits) if return_logits else indices
